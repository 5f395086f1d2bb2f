"""GPU: the masked-observation MYULA chain and SAPG estimation of theta, the PSF parameters and sigma2 (sbtv_myula_masked,
sbtv_SAPG_masked, csrc/sapg_masked.hip) against the NumPy restatement
(tests/masked_sapg_restatement.py) on the cases of tests/masked_sapg_cases.py: samples 12, warmup 4, burnIn 8.

Parity with injected noise at the bars of tests/test_gpu_sapg_skrock.py: thetas, sigmas, logpi, logpi_wu[1:] and grad_theta at
rtol 1e-9, the PSF parameters at 1e-8, their gradients and grad_sigma (a difference of two nearly equal terms) at rtol 1e-6 with
atol 1e-6 of their maximum, gx[:-1] at 1e-10, the last sample at rtol = atol = 1e-8, the EB means at 1e-9.
tests/test_masked_sapg_cpu.py shows that no prox call of a case sits on the edge of the stop rule, which is what makes the bars
meaningful.  Every test prints its figures.

Measured on an MI355X, maxima over the seven cases: thetas 1.1e-16, sigmas 3.3e-16, logpi 1.1e-14, logpi_wu 2.2e-15, grad_theta
1.6e-15, PSF parameters 9.5e-14, PSF gradients 1.5e-13 of their maximum, grad_sigma 3.0e-15, gx 4.4e-16, EB means 1.4e-14, last
sample 1.7e-13 absolute = 8.7e-16 max|X|; with m = 1 against the circular entry: traces 1.9e-15, PSF gradients 1.7e-14 of their
maximum, last sample 4.4e-16 max|X|; moments: means off by <= 1.7e-13, variances by <= 3.7e-13 relative; myula_masked: 8.4e-16
max|X|.  The whole file takes 3 s."""
import ctypes as C

import numpy as np
import pytest

import masked_sapg_cases as msc
import philox_restatement as phr
import wavelet_myula_restatement as wmr

pytestmark = pytest.mark.gpu

ARRAYS = ("thetas", "sigmas", "logPiTraceX", "logPiTrace_WU", "gXTrace", "grad_theta", "grad_sigma", "Xlast_sample")
SAPG_OF = {"gaussian": "SAPG_algorithm_Guassian", "moffat": "SAPG_algorithm_moffat", "laplace": "SAPG_algorithm_laplace"}


def _run(ctx, name, noise=None, x0=None, posterior=None, y=None, mask=None, c=None, **opkw):
    """sbtv.SAPG_masked on a case: (the tuple it returns, the problem)."""
    import sbtv
    q = msc.problem(name)
    op = dict(q["op"], **opkw)
    out = sbtv.SAPG_masked(q["kind"], q["setup"]["y"] if y is None else y, q["mask"] if mask is None else mask, op,
                           q["c"] if c is None else c, noise=noise, x0=x0, posterior=posterior, ctx=ctx)
    return out, q


def _keys(kind):
    nm = msc.NAMES_OF[kind]
    return ARRAYS + tuple(n + "s" for n in nm) + tuple("grad_" + n for n in nm)


def _same(kind, a, b, extra=()):
    for k in _keys(kind) + tuple(extra):
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
    for k in ("theta_EB", "sigma_EB") + tuple(n + "_EB" for n in msc.NAMES_OF[kind]):
        assert a[k] == b[k], k


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nz = b != 0
    return float(np.max(np.abs(a[nz] / b[nz] - 1))) if np.any(nz) else 0.0


def _as_ref(kind, out):
    """The tuple a mirror returns in the form of the restatement's dict."""
    res, nm = out[-1], msc.NAMES_OF[kind]
    return dict(thetas=res["thetas"], sigmas=res["sigmas"], logpi=res["logPiTraceX"],
                logpi_wu=np.asarray(res["logPiTrace_WU"]), gx=res["gXTrace"], ps=[res[n + "s"] for n in nm],
                grads=[res["grad_theta"]] + [res["grad_" + n] for n in nm] + [res["grad_sigma"]], theta_EB=out[0],
                sigma_EB=out[-2], p_EB=[out[1 + i] for i in range(len(nm))], samples=[np.asarray(res["Xlast_sample"])])


def _assert_parity(tag, out, kind, ref):
    res = out[-1]
    nm = msc.NAMES_OF[kind]
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
@pytest.mark.parametrize("name", msc.NAMES)
def test_traces_estimates_and_last_sample_match_the_restatement(ctx, name):
    out, q = _run(ctx, name, msc.problem(name)["noise"])
    _assert_parity(name, out, q["kind"], msc.reference(name))


# ---- 2. m = 1: the circular entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gauss-valid", "moffat-holes", "laplace-weights"])
def test_with_a_mask_of_ones_the_chain_is_that_of_the_circular_entry(ctx, name):
    """Against sbtv.SAPG_algorithm_* on the GPU with the same noise, at the bars of the parity test: spatial sums against
    Parseval sums, so not bit for bit."""
    import sbtv
    q = msc.problem(name)
    out, _ = _run(ctx, name, q["noise"], mask=np.ones_like(q["mask"]))
    circ = getattr(sbtv, SAPG_OF[q["kind"]])(q["setup"]["y"], q["op"], q["c"], noise=q["noise"], ctx=ctx)
    _assert_parity(f"{name}, m = 1 against the circular entry", out, q["kind"], _as_ref(q["kind"], circ))


# ---- 3. y under m = 0 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gauss-valid", "laplace-weights", "gauss-fixed"])
def test_y_under_a_zero_of_the_mask_moves_no_bit(ctx, name):
    """x0 given; y under m = 0 set to 0 and to 1e6: every trace, the EB means, the last sample and the moments are the same
    bits.  A pass that forgot the mask shows here."""
    q = msc.problem(name)
    y, m = q["setup"]["y"], q["mask"]
    assert np.any(m == 0)
    x0 = 0.5 * y + 20.0
    post = dict(first=0, thin=2)
    extra = ("posteriormean", "posteriorvar")
    runs = [_run(ctx, name, q["noise"], x0=x0, y=np.where(m > 0, y, v), posterior=post)[0][-1] for v in (0.0, 1e6)]
    base = _run(ctx, name, q["noise"], x0=x0, posterior=post)[0][-1]
    for r in runs:
        _same(q["kind"], r, base, extra)
    assert np.all(np.isfinite(np.asarray(base["Xlast_sample"])))
    # and the mask is felt: with every pixel observed the chain is another one
    full = _run(ctx, name, q["noise"], x0=x0, mask=np.ones_like(m), posterior=post)[0][-1]
    assert np.max(np.abs(np.asarray(full["Xlast_sample"]) - np.asarray(base["Xlast_sample"]))) > 1e-3
    assert np.any(np.asarray(full["logPiTraceX"]) != np.asarray(base["logPiTraceX"]))


# ---- 4. independence ------------------------------------------------------------------------------------------------
def test_chains_of_a_batch_are_computed_as_alone(ctx):
    """Two chains with different images, masks and start values in one call are the two single calls, bit for bit: with the
    generator and with injected noise, moments included."""
    name = "moffat-holes"
    q = msc.problem(name)
    y, m = q["setup"]["y"], q["mask"]
    y2 = np.stack([y, y[::-1].copy()])
    m2 = np.stack([m, msc.valid_mask(y.shape, 7)])
    x2 = np.stack([y, 0.5 * y[::-1] + 20.0])
    nz = np.random.default_rng(3).standard_normal((q["noise"].shape[0], 2) + y.shape)
    post = dict(first=0, thin=2)
    extra = ("posteriormean", "posteriorvar")
    for noise in (None, nz):
        both, _ = _run(ctx, name, noise, x0=x2, y=y2, mask=m2, seed=5, chain_offset=2, posterior=post)
        assert len(both[-1]) == 2
        for b in range(2):
            alone, _ = _run(ctx, name, None if noise is None else noise[:, b], x0=x2[b], y=y2[b], mask=m2[b], seed=5,
                            chain_offset=2 + b, posterior=post)
            _same(q["kind"], both[-1][b], alone[-1], extra)
            assert both[-1][b]["posterior_count"] == alone[-1]["posterior_count"]
        assert both[-1][0]["thetas"][1] != both[-1][1]["thetas"][1]


# ---- 5. the generator -----------------------------------------------------------------------------------------------
def test_philox_chain_is_the_restatement_fed_with_the_restated_normals(ctx):
    """noise = NULL: pair q of chain b draws (q, step, chain_offset + b), steps counting from 0 through the warm-up and on."""
    name, seed, off = "moffat-holes", 11, 2
    q = msc.problem(name)
    M, N = q["setup"]["y"].shape
    nz = phr.as_arrays(phr.chain_normals(M * N, q["noise"].shape[0], 1, seed, off), M)[:, 0]
    a, _ = _run(ctx, name, seed=seed, chain_offset=off)
    _assert_parity("Philox", a, q["kind"], msc.chain(name, noise=nz))
    _same(q["kind"], a[-1], _run(ctx, name, seed=seed, chain_offset=off)[0][-1])          # same seed, same bits
    c, _ = _run(ctx, name, seed=seed + 1, chain_offset=off)
    assert np.max(np.abs(np.asarray(c[-1]["Xlast_sample"]) - np.asarray(a[-1]["Xlast_sample"]))) > 1e-3


# ---- 6. moments -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["moffat-holes", "moffat-rect"])
def test_sapg_moments_are_the_welford_recursion_of_the_restated_samples(ctx, name):
    q, ref = msc.problem(name), msc.reference(name)
    S = msc.SAMPLES
    plain, _ = _run(ctx, name, q["noise"])
    for first, thin in ((0, 1), (1, 1), (2, 3), (S, 1)):
        got = _run(ctx, name, q["noise"], posterior=dict(first=first, thin=thin))[0][-1]
        f = first or msc.BURNIN
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


def _myula(ctx, name, noise="case", posterior=None, **over):
    import sbtv
    q = msc.myula_problem(name)
    A = sbtv.BlurOperator(q["model"].taps(*q["p"]))
    op = dict(y=q["y"], A=A, theta_op=q["theta"], sigma2=q["s2"], samples=q["samples"], gamma=q["gam"], chambolleit=msc.CHAMBOLLEIT,
              **{"lambda": q["lam"]})
    op.update(over)
    return sbtv.myula_masked(op, q["mask"], noise=q["noise"] if isinstance(noise, str) else noise, posterior=posterior, ctx=ctx), q


# ---- 7. the fixed-parameter chain ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["moffat-holes", "moffat-rect", "tiny"])
def test_myula_masked_matches_the_restatement(ctx, name):
    got, q = _myula(ctx, name)
    ref = msc.myula_reference(name)
    ex = float(np.max(np.abs(got - ref["x"])))
    print(f"{name}: myula_masked max|X - ref| = {ex:.1e} = {ex / np.max(np.abs(ref['x'])):.1e} max|X|")
    np.testing.assert_allclose(got, ref["x"], rtol=1e-8, atol=1e-8)


def test_myula_masked_moments_philox_and_batch(ctx):
    name = "moffat-holes"
    ref = msc.myula_reference(name)
    plain, q = _myula(ctx, name)
    last = q["samples"] - 1
    for first, thin in ((0, 1), (2, 2), (last, 1)):
        got, _ = _myula(ctx, name, posterior=dict(first=first, thin=thin))
        f = first or 1
        n = (last - f) // thin + 1
        m, v = wmr.welford(list(ref["samples"][f - 1::thin]))
        assert got["count"] == n
        print(f"myula_masked ({first}, {thin}): n = {n}, mean off by {np.max(np.abs(got['mean'] - m)):.1e}, "
              f"var by {_rel(got['var'], v):.1e} relative")
        np.testing.assert_allclose(got["mean"], m, rtol=0, atol=1e-10)
        np.testing.assert_allclose(got["var"], v, rtol=1e-8, atol=0)
        np.testing.assert_array_equal(got["x"], plain)
    # the generator: the restatement fed the restated normals; the same seed gives the same bits, another seed another chain
    M, N = q["y"].shape
    nz = phr.as_arrays(phr.chain_normals(M * N, q["samples"] - 2, 1, 7, 3), M)[:, 0]
    a, _ = _myula(ctx, name, noise=None, seed=7, chain_offset=3)
    np.testing.assert_allclose(a, msc.myula_chain(name, noise=nz)["x"], rtol=1e-8, atol=1e-8)
    np.testing.assert_array_equal(a, _myula(ctx, name, noise=None, seed=7, chain_offset=3)[0])
    assert np.max(np.abs(a - _myula(ctx, name, noise=None, seed=8, chain_offset=3)[0])) > 1e-3
    # two chains with their own masks in one call are the two single calls
    import sbtv
    y2 = np.stack([q["y"], q["y"][::-1].copy()])
    m2 = np.stack([q["mask"], msc.valid_mask(q["y"].shape, 7)])
    A = sbtv.BlurOperator(q["model"].taps(*q["p"]))
    op = dict(A=A, theta_op=q["theta"], sigma2=q["s2"], samples=q["samples"], gamma=q["gam"], chambolleit=msc.CHAMBOLLEIT, seed=7,
              **{"lambda": q["lam"]})
    both = sbtv.myula_masked(dict(op, y=y2), m2, ctx=ctx)
    for b in range(2):
        np.testing.assert_array_equal(both[b], sbtv.myula_masked(dict(op, y=y2[b], chain_offset=b), m2[b], ctx=ctx))


# ---- 8. refusals ----------------------------------------------------------------------------------------------------
def _raw_call(ctx, name, opt=None, **over):
    """sbtv_SAPG_masked through ctypes with every argument valid unless overridden: (return code, outputs)."""
    from sbtv import _lib as L
    q = msc.problem(name)
    st, op, c = q["setup"], dict(q["op"]), q["c"]
    y, m = L.Images(st["y"]), L.Images(over.pop("mask_array", q["mask"]))
    M, N = y.M, y.N
    o = L.sbtv_sapg_opts()
    o.kind, o.psf_size, o.samples, o.warmup, o.burnIn = {"gaussian": 0, "moffat": 1, "laplace": 2}[q["kind"]], 7, op["samples"], op["warmup"], op["burnIn"]
    o.chambolleit, o.lambda_, o.gamma, o.th_init, o.min_th, o.max_th = op["chambolleit"], op["lambda"], op["gamma"], op["th_init"], op["min_th"], op["max_th"]
    for i, nm in enumerate(msc.NAMES_OF[q["kind"]]):
        o.p_init[i], o.p_min[i], o.p_max[i], o.p_true[i] = op[nm + "_init"], op["min_" + nm], op["max_" + nm], op[nm]
        o.fix_p[i], o.c_p[i] = op["fix_" + nm], c[nm]
    o.sigma2_true, o.sigma2_init, o.sigma2_min, o.sigma2_max = st["sigma"] ** 2, op["sigma_init"], op["sigma_min"], op["sigma_max"]
    o.d_scale, o.d_exp, o.c_theta, o.c_sigma, o.seed = op["d_scale"], op["d_exp"], c["theta"], c["sigma"], 1
    for k, v in (opt or {}).items():
        setattr(o, k, v)
    S, W = max(o.samples, 1), max(o.warmup, 1)
    mo = L.sbtv_moments_opts(0, 1, 0)
    bufs = dict(thetas=np.zeros(S), ps=np.zeros(2 * S), sigmas=np.zeros(S), logpi=np.zeros(S), logpi_wu=np.zeros(W), gx=np.zeros(S),
                grads=np.zeros(4 * S), eb=np.zeros(4), x_last=np.zeros(M * N), post_mean=np.zeros(M * N), post_var=np.zeros(M * N),
                post_count=np.zeros(1, dtype=np.int64))
    a = dict(y=y.ptr, mask=m.ptr, M=M, N=N, batch=1, op=C.byref(o), mo=C.byref(mo), **{k: L.vptr(v) for k, v in bufs.items()})
    a.update(over)
    rc = ctx.lib.sbtv_SAPG_masked(ctx.h, a["y"], a["mask"], a["M"], a["N"], a["batch"], a["op"], None, None, a["thetas"], a["ps"],
                                  a["sigmas"], a["logpi"], a["logpi_wu"], a["gx"], a["grads"], a["eb"], a["x_last"], a["mo"],
                                  a["post_mean"], a["post_var"], a["post_count"], 0)
    return rc, bufs


def test_refusals(ctx):
    """Each is refused with its code before any GPU work, and a valid call succeeds afterwards."""
    import sbtv
    name = "gauss-valid"
    q = msc.problem(name)
    S = msc.SAMPLES
    BADARG, SIZE, MAXITER, PSF = -1, -2, -3, -10
    ctx.reset_calls()
    # what sbtv_SAPG_algorithm refuses, with its codes
    for opt, code in ((dict(samples=1, burnIn=1), BADARG), (dict(warmup=-1), BADARG), (dict(burnIn=0), BADARG),
                      (dict(burnIn=S + 1), BADARG), (dict(chain_offset=-1), BADARG), (dict(iter_offset=-1), BADARG),
                      (dict(chambolleit=0), MAXITER), (dict(kind=3), PSF), (dict(psf_size=16), PSF), (dict(psf_size=0), PSF),
                      (dict(share_gradients=1), BADARG)):
        rc, _ = _raw_call(ctx, name, opt=opt)
        assert rc == code, (opt, rc)
    for over, code in ((dict(y=None), BADARG), (dict(op=None), BADARG), (dict(batch=0), BADARG), (dict(M=33, N=35), SIZE),
                       (dict(mask=None), BADARG)):
        rc, _ = _raw_call(ctx, name, **over)
        assert rc == code, (over, rc)
    # the mask: a negative entry, a NaN, an infinity, no observed pixel
    for v in (-0.5, float("nan"), float("inf")):
        bad = q["mask"].copy()
        bad[5, 7] = v
        rc, _ = _raw_call(ctx, name, mask_array=bad)
        assert rc == BADARG, v
        with pytest.raises(sbtv.SbtvError) as e:
            _run(ctx, name, mask=bad)
        assert e.value.code == BADARG, v
    rc, _ = _raw_call(ctx, name, mask_array=np.zeros_like(q["mask"]))
    assert rc == BADARG
    with pytest.raises(sbtv.SbtvError) as e:                              # one chain of a batch without an observed pixel
        _run(ctx, name, y=np.stack([q["setup"]["y"]] * 2), mask=np.stack([q["mask"], np.zeros_like(q["mask"])]))
    assert e.value.code == BADARG
    # the moments
    for over in (dict(post_mean=None), dict(mo=None), dict(mo=None, post_mean=None, post_var=None),
                 dict(mo=None, post_mean=None, post_count=None)):
        rc, _ = _raw_call(ctx, name, **over)
        assert rc == BADARG, (over, rc)
    for post in (dict(thin=0), dict(first=S + 1), dict(first=-1)):
        with pytest.raises(sbtv.SbtvError) as e:
            _run(ctx, name, posterior=post)
        assert e.value.code == BADARG, post
    with pytest.raises(sbtv.SbtvError) as e:
        _run(ctx, name, y=np.stack([q["setup"]["y"]] * 2), mask=np.stack([q["mask"]] * 2), posterior=dict(pooled=True))
    assert e.value.code == BADARG
    # the fixed-parameter chain: the mask, an odd pixel count, moment outputs without options
    for bad in (np.where(q["mask"] > 0, -1.0, 0.0), np.full_like(q["mask"], np.nan), np.zeros_like(q["mask"])):
        mq = msc.myula_problem(name)
        A = sbtv.BlurOperator(q["model"].taps(*mq["p"]))
        with pytest.raises(sbtv.SbtvError) as e:
            sbtv.myula_masked(dict(y=mq["y"], A=A, theta_op=mq["theta"], sigma2=mq["s2"], samples=mq["samples"], gamma=mq["gam"],
                                   **{"lambda": mq["lam"]}), bad, ctx=ctx)
        assert e.value.code == BADARG
    from sbtv import _lib as L
    mq = msc.myula_problem(name)
    yi, mi = L.Images(mq["y"]), L.Images(mq["mask"])
    taps = np.ascontiguousarray(q["model"].taps(*mq["p"]).T)
    th, s2 = np.array([mq["theta"]]), np.array([mq["s2"]])
    xo, pmn = np.zeros(yi.M * yi.N), np.zeros(yi.M * yi.N)
    raw = lambda mask, M, N, pm: ctx.lib.sbtv_myula_masked(ctx.h, yi.ptr, mask, M, N, 1, L.vptr(taps), 7, mq["lam"], mq["gam"],
                                                           L.vptr(th), L.vptr(s2), mq["samples"], msc.CHAMBOLLEIT, 1, 0, None,
                                                           L.vptr(xo), None, pm, None, None, 0)
    assert raw(None, yi.M, yi.N, None) == BADARG
    assert raw(mi.ptr, 33, 35, None) == SIZE
    assert raw(mi.ptr, yi.M, yi.N, L.vptr(pmn)) == BADARG
    assert ctx.calls == 0
    assert raw(mi.ptr, yi.M, yi.N, None) == 0 and np.all(np.isfinite(xo))
    rc, bufs = _raw_call(ctx, name)
    assert rc == 0 and bufs["post_count"][0] == S - msc.BURNIN + 1 and np.all(np.isfinite(bufs["logpi"]))
    assert ctx.calls == 0                                                 # the operator layer counts nothing (include/sbtv.h)
    rc, opt = _raw_call(ctx, name, mo=None, post_mean=None, post_var=None, post_count=None, thetas=None, ps=None, sigmas=None,
                        logpi_wu=None, gx=None, grads=None, x_last=None)
    assert rc == 0
    np.testing.assert_array_equal(opt["logpi"], bufs["logpi"])           # optional outputs change nothing
    np.testing.assert_array_equal(opt["eb"], bufs["eb"])


# ---- 9. the start ---------------------------------------------------------------------------------------------------
def test_without_x0_the_chain_starts_from_y_as_given_and_no_warmup_works(ctx):
    name = "laplace-weights"
    q = msc.problem(name)
    y, m = q["setup"]["y"], q["mask"]
    yp = np.where(m > 0, y, 300.0)                                        # y under m = 0 IS the start there
    nz = q["noise"][:msc.SAMPLES - 1]
    out, _ = _run(ctx, name, nz, y=yp, warmup=0)
    _assert_parity("x0 = NULL, no warm-up", out, q["kind"], msc.chain(name, noise=nz, y=yp, warmup=0))
    other, _ = _run(ctx, name, nz, warmup=0)
    assert np.any(np.asarray(other[-1]["thetas"]) != np.asarray(out[-1]["thetas"]))
    x0 = 0.5 * y + 20.0
    out, _ = _run(ctx, name, nz, x0=x0, warmup=0)
    _assert_parity("x0, no warm-up", out, q["kind"], msc.chain(name, noise=nz, x0=x0, warmup=0))
