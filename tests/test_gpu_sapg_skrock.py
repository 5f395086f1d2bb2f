"""GPU: the SAPG estimation of theta, the PSF parameters and sigma2 with an SK-ROCK kernel (sbtv_SAPG_skrock,
csrc/sapg_skrock.hip) against the NumPy restatement (tests/sapg_skrock_restatement.py) on the cases of
tests/sapg_skrock_cases.py: samples 12, warmup 4, burnIn 8, dt = 0.8 of the stability bound at the smallest sigma2.

Parity with injected noise at the bars of test_sapg_matches_oracle_with_injected_noise: thetas, sigmas, logpi, logpi_wu[1:] and
grad_theta at rtol 1e-9, the PSF parameters at 1e-8, their gradients at rtol 1e-6 with atol 1e-6 max, gx[:-1] at 1e-10, the last
sample at rtol = atol = 1e-8, the EB means at 1e-9.  grad_sigma = R/(2 s^2) - dimX/(2 s) is a difference of two nearly equal
terms: it gets the bar of the PSF gradients.  tests/test_sapg_skrock_cpu.py shows that no prox call of a case sits on the edge
of the stop rule and how little the loop amplifies prox rounding, which is what makes the bars meaningful.  Every test prints
its figures.

Measured on an MI355X, maxima over the six cases: thetas 3.3e-16, sigmas 5.3e-15, logpi 3.0e-15, logpi_wu 1.6e-15, grad_theta
6.3e-15, PSF parameters 8.3e-14, PSF gradients 1.4e-12 of their maximum, grad_sigma 2.4e-15, gx 2.0e-15, EB means 5.7e-15, last
sample 3.0e-12 absolute = 1.4e-14 max|X| (Laplace, s = 10; <= 4.1e-15 max|X| elsewhere); moments: means off by <= 8.5e-13,
variances by <= 6.7e-13 relative; the statistic: theta_EB 0.03 and b_EB 0.11 pooled standard errors apart.  The whole file takes
7 s."""
import ctypes as C
import functools

import numpy as np
import pytest

import philox_restatement as phr
import sapg_skrock_cases as ssc
import wavelet_myula_restatement as wmr

pytestmark = pytest.mark.gpu

ARRAYS = ("thetas", "sigmas", "logPiTraceX", "logPiTrace_WU", "gXTrace", "grad_theta", "grad_sigma", "Xlast_sample")


def _run(ctx, name, noise=None, x0=None, posterior=None, y=None, c=None, stages=None, dt=None, eta=ssc.ETA, **opkw):
    """sbtv.SAPG_skrock on a case: (the tuple it returns, the problem)."""
    import sbtv
    q = ssc.problem(name)
    op = dict(q["op"], **opkw)
    out = sbtv.SAPG_skrock(q["kind"], q["setup"]["y"] if y is None else y, op, q["c"] if c is None else c,
                           q["stages"] if stages is None else stages, q["dt"] if dt is None else dt, eta, noise=noise, x0=x0,
                           posterior=posterior, ctx=ctx)
    return out, q


def _keys(kind):
    nm = ssc.NAMES_OF[kind]
    return ARRAYS + tuple(n + "s" for n in nm) + tuple("grad_" + n for n in nm)


def _same(kind, a, b, extra=()):
    for k in _keys(kind) + tuple(extra):
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
    for k in ("theta_EB", "sigma_EB") + tuple(n + "_EB" for n in ssc.NAMES_OF[kind]):
        assert a[k] == b[k], k


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nz = b != 0
    return float(np.max(np.abs(a[nz] / b[nz] - 1))) if np.any(nz) else 0.0


def _assert_parity(tag, out, kind, ref):
    res = out[-1]
    nm = ssc.NAMES_OF[kind]
    x = ref["samples"][-1]
    ex = float(np.max(np.abs(np.asarray(res["Xlast_sample"]) - x)))
    tight = [("thetas", res["thetas"], ref["thetas"]), ("sigmas", res["sigmas"], ref["sigmas"]),
             ("logpi", res["logPiTraceX"], ref["logpi"]), ("logpi_wu", res["logPiTrace_WU"][1:], ref["logpi_wu"][1:]),
             ("grad_theta", res["grad_theta"], ref["grads"][0])]
    psf = [(n + "s", res[n + "s"], ref["ps"][i]) for i, n in enumerate(nm)]
    loose = [("grad_" + n, res["grad_" + n], ref["grads"][1 + i]) for i, n in enumerate(nm)]
    loose.append(("grad_sigma", res["grad_sigma"], ref["grads"][len(nm) + 1]))
    eb = [("theta_EB", out[0], ref["theta_EB"]), ("sigma_EB", out[-2], ref["sigma_EB"])]
    eb += [(n + "_EB", out[1 + i], ref["p_EB"][i]) for i, n in enumerate(nm)]
    print(f"{tag}: " + ", ".join(f"{k} {_rel(a, b):.1e}" for k, a, b in tight + psf + eb) + f", gx {_rel(res['gXTrace'][:-1], ref['gx'][:-1]):.1e}"
          + "; gradients (abs / max) " + ", ".join(f"{k} {np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b)):.1e}" for k, a, b in loose)
          + f"; max|X - ref| = {ex:.1e} = {ex / np.max(np.abs(x)):.1e} max|X|")
    for k, a, b in tight:
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=0, err_msg=k)
    for k, a, b in psf:
        np.testing.assert_allclose(a, b, rtol=1e-8, atol=0, err_msg=k)
    for k, a, b in loose:
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-6 * np.max(np.abs(b)), err_msg=k)
    np.testing.assert_allclose(res["gXTrace"][:-1], ref["gx"][:-1], rtol=1e-10, atol=0)
    assert res["gXTrace"][-1] == 0.0
    np.testing.assert_allclose(np.asarray(res["Xlast_sample"]), x, rtol=1e-8, atol=1e-8)
    for k, a, b in eb:
        assert a == pytest.approx(b, rel=1e-9), k


# ---- 1. parity with injected noise ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ssc.NAMES)
def test_traces_estimates_and_last_sample_match_the_restatement(ctx, name):
    out, q = _run(ctx, name, ssc.problem(name)["noise"])
    _assert_parity(name, out, q["kind"], ssc.reference(name))


def test_start_state_and_no_warmup(ctx):
    """X = x0, warmup = 0: the first SAPG iteration is the first step of the call (the perturbation kernel runs there)."""
    name = "moffat-s3"
    q = ssc.problem(name)
    x0 = 0.5 * q["setup"]["y"] + 20.0
    nz = q["noise"][:ssc.SAMPLES - 1]
    out, _ = _run(ctx, name, nz, x0=x0, warmup=0)
    _assert_parity("x0, no warm-up", out, q["kind"], ssc.chain(name, noise=nz, x0=x0, warmup=0))


# ---- 2. the generator -----------------------------------------------------------------------------------------------
def test_philox_chain_is_the_restatement_fed_with_the_restated_normals(ctx):
    """noise = NULL: pair q of chain b draws (q, step, chain_offset + b), steps counting from 0 through the warm-up and on."""
    name, seed, off = "moffat-s3", 11, 2
    q = ssc.problem(name)
    M, N = q["setup"]["y"].shape
    nz = phr.as_arrays(phr.chain_normals(M * N, q["noise"].shape[0], 1, seed, off), M)[:, 0]
    a, _ = _run(ctx, name, seed=seed, chain_offset=off)
    _assert_parity("Philox", a, q["kind"], ssc.chain(name, noise=nz))
    _same(q["kind"], a[-1], _run(ctx, name, seed=seed, chain_offset=off)[0][-1])          # same seed, same bits
    c, _ = _run(ctx, name, seed=seed + 1, chain_offset=off)
    assert np.max(np.abs(np.asarray(c[-1]["Xlast_sample"]) - np.asarray(a[-1]["Xlast_sample"]))) > 1e-3


# ---- 3. frozen parameters: the fixed-parameter sampler ---------------------------------------------------------------
def test_with_everything_fixed_the_chain_is_that_of_sbtv_skrock(ctx):
    """theta = th_init, sigma2 = sigma2_init, PSF fixed at p_true, zero step scales, x0 = y, no warm-up, the same seed: x_last
    and logpi are those of sbtv_skrock, bit for bit."""
    import sbtv
    name, seed = "gauss-fixed-s3", 5
    q = ssc.problem(name)
    st, op = q["setup"], q["op"]
    zero = dict(q["c"], theta=0.0, sigma=0.0, w1=0.0, w2=0.0)
    out, _ = _run(ctx, name, c=zero, warmup=0, fix_sigma=1, seed=seed)
    res = out[-1]
    assert np.all(res["thetas"] == op["th_init"]) and np.all(res["sigmas"] == op["sigma_init"])
    A = sbtv.BlurOperator(sbtv.psf_family("gaussian", 7, st["p_true"])[0])
    sk = sbtv.skrock(dict(y=st["y"], A=A, theta_op=op["th_init"], sigma2=op["sigma_init"], samples=ssc.SAMPLES, stages=q["stages"],
                          delta=q["dt"], eta=ssc.ETA, chambolleit=ssc.CHAMBOLLEIT, seed=seed, **{"lambda": st["lam"]}), ctx=ctx)
    np.testing.assert_array_equal(np.asarray(res["Xlast_sample"]), np.asarray(sk["x"]))
    np.testing.assert_array_equal(res["logPiTraceX"], sk["logpi"])
    np.testing.assert_array_equal(res["gXTrace"][:-1], sk["gx"][1:])


# ---- 4. independence ------------------------------------------------------------------------------------------------
def test_chains_of_a_batch_are_computed_as_alone(ctx):
    """Three chains with different y and start values in one call are the three single calls, bit for bit: with the generator
    and with injected noise, moments included."""
    name = "moffat-s3"
    q = ssc.problem(name)
    y = q["setup"]["y"]
    y3 = np.stack([y, y[::-1].copy(), y.T.copy()])
    x3 = np.stack([y, 0.5 * y[::-1] + 20.0, 0.9 * y.T + 5.0])
    nz = np.random.default_rng(3).standard_normal((q["noise"].shape[0], 3) + y.shape)
    post = dict(first=0, thin=2)
    extra = ("posteriormean", "posteriorvar")
    for noise in (None, nz):
        both, _ = _run(ctx, name, noise, x0=x3, y=y3, seed=5, chain_offset=2, posterior=post)
        assert len(both[-1]) == 3
        for b in range(3):
            alone, _ = _run(ctx, name, None if noise is None else noise[:, b], x0=x3[b], y=y3[b], seed=5, chain_offset=2 + b,
                            posterior=post)
            _same(q["kind"], both[-1][b], alone[-1], extra)
            assert both[-1][b]["posterior_count"] == alone[-1]["posterior_count"]
        assert both[-1][0]["thetas"][1] != both[-1][1]["thetas"][1]


# ---- 5. moments -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["moffat-s3", "moffat-rect-s5"])
def test_moments_are_the_welford_recursion_of_the_restated_samples(ctx, name):
    q, ref = ssc.problem(name), ssc.reference(name)
    S = ssc.SAMPLES
    plain, _ = _run(ctx, name, q["noise"])
    for first, thin in ((0, 1), (1, 1), (2, 3), (S, 1)):
        got = _run(ctx, name, q["noise"], posterior=dict(first=first, thin=thin))[0][-1]
        f = first or ssc.BURNIN
        n = (S - f) // thin + 1
        m, v = wmr.welford(list(ref["samples"][f - 1::thin]))
        assert got["posterior_count"] == n
        print(f"{name} ({first}, {thin}): n = {n}, mean off by {np.max(np.abs(got['posteriormean'] - m)):.1e}, "
              f"var by {_rel(got['posteriorvar'], v):.1e} relative (max var {np.max(v):.3g})")
        np.testing.assert_allclose(got["posteriormean"], m, rtol=0, atol=1e-10)
        np.testing.assert_allclose(got["posteriorvar"], v, rtol=1e-8, atol=0)
        _same(q["kind"], got, plain[-1])                                 # moments change no bit of the chain or its traces
        if n == 1:
            assert not np.any(got["posteriorvar"])


# ---- 6. device pointers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gauss-s2", "moffat-s3"])
def test_device_tensors_give_the_same_bits(ctx, name):
    """Both parities of the stage count: the last sample ends in the caller's buffer or in the second one."""
    import sbtv
    q = ssc.problem(name)
    y = q["setup"]["y"]
    post = dict(first=2, thin=2)
    x0 = 0.5 * y + 20.0
    host = _run(ctx, name, q["noise"], x0=x0, posterior=post)[0][-1]
    dev = _run(ctx, name, sbtv.to_device(q["noise"]), x0=sbtv.to_device(x0), posterior=post, y=sbtv.to_device(y))[0][-1]
    assert dev["posterior_count"] == host["posterior_count"]
    for k in ("Xlast_sample", "posteriormean", "posteriorvar"):
        assert dev[k].is_cuda
        np.testing.assert_array_equal(sbtv.to_host(dev[k]), np.asarray(host[k]), err_msg=k)
        dev[k] = sbtv.to_host(dev[k])
    _same(q["kind"], dev, host)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def _raw_call(ctx, name, opt=None, step=None, **over):
    """sbtv_SAPG_skrock through ctypes with every argument valid unless overridden: (return code, outputs)."""
    from sbtv import _lib as L
    q = ssc.problem(name)
    st, op, c = q["setup"], dict(q["op"]), q["c"]
    y = L.Images(st["y"])
    M, N = y.M, y.N
    o = L.sbtv_sapg_opts()
    o.kind, o.psf_size, o.samples, o.warmup, o.burnIn = {"gaussian": 0, "moffat": 1, "laplace": 2}[q["kind"]], 7, op["samples"], op["warmup"], op["burnIn"]
    o.chambolleit, o.lambda_, o.th_init, o.min_th, o.max_th = op["chambolleit"], op["lambda"], op["th_init"], op["min_th"], op["max_th"]
    for i, nm in enumerate(ssc.NAMES_OF[q["kind"]]):
        o.p_init[i], o.p_min[i], o.p_max[i], o.p_true[i] = op[nm + "_init"], op["min_" + nm], op["max_" + nm], op[nm]
        o.fix_p[i], o.c_p[i] = op["fix_" + nm], c[nm]
    o.sigma2_true, o.sigma2_init, o.sigma2_min, o.sigma2_max = st["sigma"] ** 2, op["sigma_init"], op["sigma_min"], op["sigma_max"]
    o.d_scale, o.d_exp, o.c_theta, o.c_sigma, o.seed = op["d_scale"], op["d_exp"], c["theta"], c["sigma"], 1
    for k, v in (opt or {}).items():
        setattr(o, k, v)
    s = dict(stages=q["stages"], dt=q["dt"], eta=ssc.ETA)
    s.update(step or {})
    stp = L.sbtv_sapg_skrock_step(s["stages"], s["dt"], s["eta"])
    S, W = max(o.samples, 1), max(o.warmup, 1)
    mo = L.sbtv_moments_opts(0, 1, 0)
    bufs = dict(thetas=np.zeros(S), ps=np.zeros(2 * S), sigmas=np.zeros(S), logpi=np.zeros(S), logpi_wu=np.zeros(W), gx=np.zeros(S),
                grads=np.zeros(4 * S), eb=np.zeros(4), x_last=np.zeros(M * N), post_mean=np.zeros(M * N), post_var=np.zeros(M * N),
                post_count=np.zeros(1, dtype=np.int64))
    a = dict(y=y.ptr, M=M, N=N, batch=1, op=C.byref(o), sk=C.byref(stp), mo=C.byref(mo), **{k: L.vptr(v) for k, v in bufs.items()})
    a.update(over)
    rc = ctx.lib.sbtv_SAPG_skrock(ctx.h, a["y"], a["M"], a["N"], a["batch"], a["op"], a["sk"], None, None, a["thetas"], a["ps"],
                                  a["sigmas"], a["logpi"], a["logpi_wu"], a["gx"], a["grads"], a["eb"], a["x_last"], a["mo"],
                                  a["post_mean"], a["post_var"], a["post_count"], 0)
    return rc, bufs


def test_refusals(ctx):
    """Each is refused with its code before any GPU work, and a valid call succeeds afterwards."""
    import sbtv
    name = "gauss-s2"
    S = ssc.SAMPLES
    nan, inf = float("nan"), float("inf")
    BADARG, SIZE, MAXITER, PSF = -1, -2, -3, -10
    ctx.reset_calls()
    # what sbtv_SAPG_algorithm refuses, with its codes
    for opt, code in ((dict(samples=1, burnIn=1), BADARG), (dict(warmup=-1), BADARG), (dict(burnIn=0), BADARG),
                      (dict(burnIn=S + 1), BADARG), (dict(chain_offset=-1), BADARG), (dict(iter_offset=-1), BADARG),
                      (dict(chambolleit=0), MAXITER), (dict(chambolleit=-2), MAXITER), (dict(kind=3), PSF), (dict(kind=-1), PSF),
                      (dict(psf_size=16), PSF), (dict(psf_size=0), PSF), (dict(psf_size=33), PSF),
                      (dict(share_gradients=1), BADARG)):
        rc, _ = _raw_call(ctx, name, opt=opt)
        assert rc == code, (opt, rc)
    for over, code in ((dict(y=None), BADARG), (dict(op=None), BADARG), (dict(batch=0), BADARG), (dict(M=33, N=35), SIZE),
                       (dict(sk=None), BADARG)):
        rc, _ = _raw_call(ctx, name, **over)
        assert rc == code, (over, rc)
    # the step
    bad = [dict(stages=1), dict(stages=0), dict(stages=-3)]
    for f in ("dt", "eta"):
        bad += [{f: 0.0}, {f: -1.0}, {f: nan}, {f: inf}]
    for sk in bad:
        rc, _ = _raw_call(ctx, name, step=sk)
        assert rc == BADARG, (sk, rc)
        with pytest.raises(sbtv.SbtvError) as e:
            _run(ctx, name, **sk)
        assert e.value.code == BADARG, sk
    # the moments
    for over in (dict(post_mean=None), dict(mo=None), dict(mo=None, post_mean=None, post_var=None),
                 dict(mo=None, post_mean=None, post_count=None)):
        rc, _ = _raw_call(ctx, name, **over)
        assert rc == BADARG, (over, rc)
    for post in (dict(thin=0), dict(first=S + 1), dict(first=-1)):
        with pytest.raises(sbtv.SbtvError) as e:
            _run(ctx, name, posterior=post)
        assert e.value.code == BADARG, post
    y = ssc.problem(name)["setup"]["y"]
    with pytest.raises(sbtv.SbtvError) as e:
        _run(ctx, name, y=np.stack([y, y]), posterior=dict(pooled=True))
    assert e.value.code == BADARG
    assert ctx.calls == 0
    rc, bufs = _raw_call(ctx, name)
    assert rc == 0 and bufs["post_count"][0] == S - ssc.BURNIN + 1 and np.all(np.isfinite(bufs["logpi"]))
    assert ctx.calls == 0                                                 # the operator layer counts nothing (include/sbtv.h)
    rc, opt = _raw_call(ctx, name, mo=None, post_mean=None, post_var=None, post_count=None, thetas=None, ps=None, sigmas=None,
                        logpi_wu=None, gx=None, grads=None, x_last=None)
    assert rc == 0
    np.testing.assert_array_equal(opt["logpi"], bufs["logpi"])           # optional outputs change nothing
    np.testing.assert_array_equal(opt["eb"], bufs["eb"])


# ---- 8. statistics --------------------------------------------------------------------------------------------------
STAT_CHAINS, STAT = 8, dict(samples=60, warmup=10, burnIn=20)


@functools.lru_cache(maxsize=None)
def _stat_reference():
    """theta_EB and b_EB of 8 restatement chains on the Laplace case at s = 10, NumPy normals (computed once)."""
    q = ssc.problem("laplace-s10")
    shape = (STAT["warmup"] - 1 + STAT["samples"] - 1,) + q["setup"]["y"].shape
    rs = [ssc.chain("laplace-s10", noise=np.random.default_rng(100 + c).standard_normal(shape), **STAT) for c in range(STAT_CHAINS)]
    return np.array([r["theta_EB"] for r in rs]), np.array([r["p_EB"][0] for r in rs])


def test_estimates_of_philox_chains_within_the_restatement_chains_spread(ctx):
    """8 device Philox chains against 8 restatement chains with NumPy normals: |difference of the group means| of theta_EB and
    of b_EB <= 3 pooled standard errors, the rule of test_gx_of_philox_chains_within_the_restatement_chains_spread."""
    q = ssc.problem("laplace-s10")
    y8 = np.repeat(q["setup"]["y"][None], STAT_CHAINS, axis=0)
    out, _ = _run(ctx, "laplace-s10", y=y8, seed=7, **STAT)
    n = STAT_CHAINS
    for what, gpu, ref in zip(("theta_EB", "b_EB"), (np.array(out[0]), np.array(out[1])), _stat_reference()):
        assert len(set(gpu.tolist())) == n                                              # all different streams
        se = np.sqrt(gpu.var(ddof=1) / n + ref.var(ddof=1) / n)
        diff = abs(gpu.mean() - ref.mean())
        print(f"mean {what}: device {gpu.mean():.8g} (spread {gpu.std(ddof=1) / gpu.mean():.2e}), restatement {ref.mean():.8g} "
              f"(spread {ref.std(ddof=1) / ref.mean():.2e}), |d| = {diff:.3g}, z = {diff / se:.2f} SE")
        assert diff <= 3.0 * se
