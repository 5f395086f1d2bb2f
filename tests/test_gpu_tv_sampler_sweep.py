"""GPU: sbtv_skrock, sbtv_SAPG_skrock, sbtv_myula_masked and sbtv_SAPG_masked at the image geometries of
tests/tv_sampler_geometry_cases.py against their NumPy restatements: the wave FFT plan with two grid-stride trips of every lane
and four-trip totals (1024 x 1024), one lane on a second trip over the chirp-z path with more than 256 tvnorm_partials
(1090 x 481), rectangular power-of-two plans (256 x 64, 64 x 256), the partial-wave row pass (16 x 16), odd M (25 x 40) and
fewer pairs than one wave (8 x 8).  tests/test_tv_sampler_geometry_cases_cpu.py shows that the table reaches those classes, that
no prox call of a case sits on the edge of the stop rule and that the chains amplify prox rounding by less than 1e3, which is
what makes the bars meaningful.

Bars, those the drivers' own files hold for the same quantities (tests/test_gpu_skrock_tv.py, test_gpu_sapg_skrock.py,
test_gpu_sapg_masked.py, test_gpu_posterior.py), unchanged: the last sample at rtol = atol = 1e-9; gx and logpi of sbtv_skrock at
rtol 1e-9; SAPG: thetas, sigmas, logpi, logpi_wu[1:], grad_theta at rtol 1e-9, the PSF parameters at 1e-8, their gradients and
grad_sigma at rtol 1e-6 with atol 1e-6 of their maximum, gx[:-1] at 1e-10, the EB means at 1e-9; moments: means at rtol = atol =
1e-8, variances at rtol 1e-6 with atol 1e-8 of their maximum.  Everything that compares the library with itself (a batch
against single calls, one call against a restarted one, a run against its repetition) is bit for bit.

Which test catches which slip (read from csrc/skrock_stage.inc, skrock.hip, sapg_skrock.hip, sapg_masked.hip,
sapg_chain_update.inc):
  a grid stride of gridDim.x*256 - 1      the second trip lands one pair early, so a pair is done by two lanes.
                                          masked_resid_kernel then counts that pair twice in R (and in the derivative sums)
                                          whatever the order of the two lanes: logpi, grad_sigma and the sigma2 step of
                                          SAPG_masked at wave and seam.  The in-place stage kernels (K_j over V, P_next over U,
                                          the Welford update) apply their update twice unless both lanes read before either
                                          writes: parity and the moments test at wave and seam, the latter by name on the pixels
                                          beyond 524 288.  A stride one too long is deterministic everywhere: at seam pair 262 144
                                          is never written
  q reset / wrong on the second trip      the Philox test at the seam: pair 262 144 would draw pair 0's counter (the test shows
                                          that this moves the last pair of the sample by about 5); an address formed from a
                                          reset q leaves the second half of a 1024 x 1024 image unwritten: parity at wave.  With
                                          injected noise the counter does not show, which is why that test runs the generator
  ntv taken for nrb (or the reverse)      parity of gx / logpi at wave (ntv 1024, nrb 128), at seam (ntv 279, nrb 256) and at the
                                          rectangular plans, in all three trace-bearing drivers; masked: nblk 1024 against ntv
  a `part` slot stride without `batch`    the batch-of-two tests at seam and oddM (chirp-z: skrock.hip lays the ring out as
                                          part + slot*batch*ntv): slot 1 would start inside slot 0, over chain 1's partials
  ii0 off by one after the ring flush     the trace-ring test: the entries of the second flush (samples 1025 .. 1030) of the single
                                          call would land one entry off against the restarted call, whose rings never fill

Measured on an MI355X, worst over the cases.  sbtv_skrock: gx 6.7e-16, logpi 1.3e-14 (8 x 8; <= 2.3e-15 elsewhere), last sample
2.3e-15 max|X| (6.0e-13 absolute); with the generator at the seam 2.2e-16 / 2.0e-15 / 2.2e-15 max|X|.  sbtv_SAPG_skrock: thetas
2.2e-16, sigmas 0, logpi 2.7e-15, logpi_wu 1.8e-15, grad_theta 3.2e-15, PSF parameters 8.9e-16, PSF gradients 7.7e-14 of their
maximum, grad_sigma 2.9e-15, gx 3.3e-16, EB means 7.8e-16, last sample 2.6e-15 max|X|.  sbtv_SAPG_masked: thetas 2.2e-16, sigmas
6.7e-16, logpi 3.1e-15, logpi_wu 1.1e-15, grad_theta 4.3e-15, PSF parameters 5.5e-13 (Laplace b under scattered holes at 1024 x
1024; <= 6.4e-15 elsewhere), PSF gradients 1.6e-13 of their maximum, grad_sigma 1.2e-15, gx 6.7e-16, EB means 3.0e-13, last
sample 7.9e-16 max|X|.  sbtv_myula_masked: last sample 2.1e-15 max|X|.  Moments: means off by <= 6.3e-13 absolute, variances by
<= 2.9e-14 of their maximum.  Every bit-for-bit comparison held.  The whole file takes 15 s; its slowest tests are the parity
tests at 1024 x 1024 (0.9 - 1.2 s each, nearly all of it the CPU reference); the two 1030-iteration SAPG runs take 0.3 s each,
so that part is not skipped."""
import numpy as np
import pytest

import fft_plan_cases as fpc
import masked_sapg_cases as msc
import philox_restatement as phr
import sapg_skrock_cases as ssc
import skrock_tv_cases as skc
import tv_sampler_geometry_cases as gc
import wavelet_myula_restatement as wmr

pytestmark = pytest.mark.gpu

SECOND_TRIP = 2 * gc.EW_MAX_BLOCKS * gc.EW_LANES          # 524 288: the first double a lane writes on its second trip
BATCH_TAGS = {"skrock": ("wave", "seam", "oddM"), "SAPG_skrock": ("wave", "seam", "oddM"),
              "SAPG_masked": ("wave-holes", "seam-valid", "oddM"), "myula_masked": ("wave-valid", "seam-holes", "oddM")}
NAMES_OF = ssc.NAMES_OF
SAPG_ARRAYS = ("thetas", "sigmas", "logPiTraceX", "logPiTrace_WU", "gXTrace", "grad_theta", "grad_sigma", "Xlast_sample")
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nz = b != 0
    return float(np.max(np.abs(a[nz] / b[nz] - 1))) if np.any(nz) else 0.0


# ---- the four entries on a problem of tests/tv_sampler_geometry_cases.py ------------------------------------------------
def _skrock(ctx, q, noise=None, x0=None, posterior=None, **kw):
    import sbtv
    A = sbtv.BlurOperator(sbtv.psf_family("gaussian", 7, q["p"])[0])
    op = dict(dict(q["op"], y=q["y"], A=A, theta_op=q["theta"], sigma2=q["sigma2"]), **kw)
    return sbtv.skrock(op, noise=noise, x0=x0, posterior=posterior, ctx=ctx)


def _sapg_skrock(ctx, q, noise=None, x0=None, posterior=None, y=None, **opkw):
    import sbtv
    return sbtv.SAPG_skrock(q["kind"], q["setup"]["y"] if y is None else y, dict(q["op"], **opkw), q["c"], q["stages"], q["dt"],
                            ssc.ETA, noise=noise, x0=x0, posterior=posterior, ctx=ctx)


def _sapg_masked(ctx, q, noise=None, x0=None, posterior=None, y=None, mask=None, **opkw):
    import sbtv
    return sbtv.SAPG_masked(q["kind"], q["setup"]["y"] if y is None else y, q["mask"] if mask is None else mask,
                            dict(q["op"], **opkw), q["c"], noise=noise, x0=x0, posterior=posterior, ctx=ctx)


def _myula_masked(ctx, q, noise=None, posterior=None, mask=None, **kw):
    import sbtv
    A = sbtv.BlurOperator(q["model"].taps(*q["p"]))
    op = dict(y=q["y"], A=A, theta_op=q["theta"], sigma2=q["s2"], samples=q["samples"], gamma=q["gam"],
              chambolleit=q["chambolleit"], **{"lambda": q["lam"]})
    op.update(kw)
    return sbtv.myula_masked(op, q["mask"] if mask is None else mask, noise=noise, posterior=posterior, ctx=ctx)


# ---- the bars ---------------------------------------------------------------------------------------------------------
def _assert_last_sample(tag, x, ref):
    ex, xs = float(np.max(np.abs(np.asarray(x) - ref))), float(np.max(np.abs(ref)))
    print(f"{tag}: max|X - ref| = {ex:.1e} = {ex / xs:.1e} max|X|")
    _note(tag.split()[0] + " last sample / max|X|", ex / xs)
    np.testing.assert_allclose(np.asarray(x), ref, rtol=1e-9, atol=1e-9)


def _assert_skrock(tag, r, rr):
    for k in ("gx", "logpi"):
        a = np.asarray(r[k])
        assert a.shape == rr[k].shape, (k, a.shape)
        print(f"{tag} {k}: worst rel {_rel(a, rr[k]):.1e}")
        _note("skrock " + k, _rel(a, rr[k]))
    _assert_last_sample(tag, r["x"], rr["samples"][-1])
    for k in ("gx", "logpi"):
        np.testing.assert_allclose(np.asarray(r[k]), rr[k], rtol=1e-9, atol=0, err_msg=k)


def _sapg_pairs(res, eb_out, kind, ref, n=None):
    """(tight, psf, loose, eb): (name, got, reference) of the first n iterations (all: n = None)."""
    nm = NAMES_OF[kind]
    s = slice(None, n)
    tight = [("thetas", res["thetas"][s], ref["thetas"][s]), ("sigmas", res["sigmas"][s], ref["sigmas"][s]),
             ("logpi", res["logPiTraceX"][s], ref["logpi"][s]), ("logpi_wu", res["logPiTrace_WU"][1:], ref["logpi_wu"][1:]),
             ("grad_theta", res["grad_theta"][s], ref["grads"][0][s])]
    psf = [(n_ + "s", res[n_ + "s"][s], ref["ps"][i][s]) for i, n_ in enumerate(nm)]
    loose = [("grad_" + n_, res["grad_" + n_][s], ref["grads"][1 + i][s]) for i, n_ in enumerate(nm)]
    loose.append(("grad_sigma", res["grad_sigma"][s], ref["grads"][len(nm) + 1][s]))
    eb = []
    if eb_out is not None:
        eb = [("theta_EB", eb_out[0], ref["theta_EB"]), ("sigma_EB", eb_out[-2], ref["sigma_EB"])]
        eb += [(n_ + "_EB", eb_out[1 + i], ref["p_EB"][i]) for i, n_ in enumerate(nm)]
    return tight, psf, loose, eb


def _assert_sapg_traces(tag, driver, res, eb_out, kind, ref, n=None):
    """The bars of tests/test_gpu_sapg_skrock.py / test_gpu_sapg_masked.py on the traces of the first n iterations."""
    tight, psf, loose, eb = _sapg_pairs(res, eb_out, kind, ref, n)
    gx_got, gx_ref = (res["gXTrace"][:-1], ref["gx"][:-1]) if n is None else (res["gXTrace"][:n - 1], ref["gx"][:n - 1])
    print(f"{tag}: " + ", ".join(f"{k} {_rel(a, b):.1e}" for k, a, b in tight + psf + eb) + f", gx {_rel(gx_got, gx_ref):.1e}"
          + "; gradients (abs / max) "
          + ", ".join(f"{k} {np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b)):.1e}" for k, a, b in loose))
    for k, a, b in tight + eb:
        _note(f"{driver} {k}", _rel(a, b))
    for k, a, b in psf:
        _note(f"{driver} PSF parameters", _rel(a, b))
    for k, a, b in loose:
        _note(f"{driver} {'grad_sigma' if k == 'grad_sigma' else 'PSF gradients'} / max",
              np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b)))
    _note(f"{driver} gx", _rel(gx_got, gx_ref))
    for k, a, b in tight:
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=0, err_msg=k)
    for k, a, b in psf:
        np.testing.assert_allclose(a, b, rtol=1e-8, atol=0, err_msg=k)
    for k, a, b in loose:
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-6 * np.max(np.abs(b)), err_msg=k)
    np.testing.assert_allclose(gx_got, gx_ref, rtol=1e-10, atol=0)
    for k, a, b in eb:
        assert a == pytest.approx(b, rel=1e-9), k


def _assert_sapg(tag, driver, out, kind, ref):
    res = out[-1]
    _assert_sapg_traces(tag, driver, res, out, kind, ref)
    assert res["gXTrace"][-1] == 0.0
    _assert_last_sample(tag, res["Xlast_sample"], ref["samples"][-1])


def _assert_moments(tag, mean, var, samples):
    """The tolerance of tests/test_gpu_posterior.py, on all pixels and, by name, on those a lane writes on its second
    grid-stride trip (doubles 524 288 and beyond of the image in device memory), where there are any."""
    m, v = wmr.welford(list(samples))
    mean, var = np.asarray(mean), np.asarray(var)
    dm, dv = np.max(np.abs(mean - m)), np.max(np.abs(var - v))
    print(f"{tag}: n = {len(samples)}, mean off by {dm:.1e}, var by {dv:.1e} (max var {np.max(v):.3g})")
    _note(tag.split()[0] + " moments: mean (abs)", dm)
    _note(tag.split()[0] + " moments: var / max var", dv / max(np.max(v), 1e-300))
    parts = [("all pixels", slice(None))]
    if mean.size > SECOND_TRIP:
        parts.append(("second trip", slice(SECOND_TRIP, None)))
    for what, s in parts:
        a, b, c, d = (phr.device_order(t)[s] for t in (mean, m, var, v))
        np.testing.assert_allclose(a, b, rtol=1e-8, atol=1e-8, err_msg=f"mean, {what}")
        np.testing.assert_allclose(c, d, rtol=1e-6, atol=1e-8 * np.max(v), err_msg=f"var, {what}")
    if len(samples) > 1:
        assert np.any(phr.device_order(var)[-2:] > 0)                    # the last pair has been accumulated at all
    return len(samples)


# ---- 0. the model of the geometry is the library's ----------------------------------------------------------------------
def test_the_library_reports_the_plans_and_tiles_the_case_table_is_built_on(ctx):
    shapes = sorted({gc.shape(d, t) for d, t in gc.ALL})
    for M, N in shapes:
        for batch in (1, 2):
            plan = ctx.fft_plan(M, N, batch)
            assert plan == fpc.model_plan(M, N, batch), (M, N, batch, plan)
        pg, pv = ctx.prox_geometry(M, N), ctx.prox_variant(M, N)
        assert (pg["single_ti"], pg["single_tj"]) == gc.TVNORM_TILE
        assert pv["fused"] == (M % 2 == 0), (M, N, pv)                   # odd M: the one-iteration (scalar) kernels
        print(f"{M} x {N}: {gc.geometry(M, N)['plan_class']}, prox rows_per_lane {pg['rows_per_lane']}, tiles "
              f"{pg['tiles_i']} x {pg['tiles_j']}, tile table {pg['order']}")
    big, small = ctx.prox_geometry(1024, 1024), ctx.prox_geometry(256, 64)
    assert big["rows_per_lane"] == 2 and big["tiles_i"] * big["tiles_j"] >= 256 and small["rows_per_lane"] == 1
    assert ctx.prox_geometry(1024, 1024, 2)["rows_per_lane"] == 2
    for d in gc.DRIVERS:
        gc.assert_reaches(d)


# ---- 1. parity with injected noise --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(gc.SKROCK))
def test_skrock_matches_the_restatement(ctx, tag):
    q = gc.problem("skrock", tag)
    _assert_skrock(f"skrock {tag}", _skrock(ctx, q, q["noise"]), gc.reference("skrock", tag))


@pytest.mark.parametrize("tag", list(gc.SAPG_SKROCK))
def test_sapg_skrock_matches_the_restatement(ctx, tag):
    q = gc.problem("SAPG_skrock", tag)
    _assert_sapg(f"SAPG_skrock {tag}", "SAPG_skrock", _sapg_skrock(ctx, q, q["noise"]), q["kind"], gc.reference("SAPG_skrock", tag))


@pytest.mark.parametrize("tag", list(gc.SAPG_MASKED))
def test_sapg_masked_matches_the_restatement(ctx, tag):
    q = gc.problem("SAPG_masked", tag)
    _assert_sapg(f"SAPG_masked {tag}", "SAPG_masked", _sapg_masked(ctx, q, q["noise"]), q["kind"], gc.reference("SAPG_masked", tag))


@pytest.mark.parametrize("tag", list(gc.MYULA_MASKED))
def test_myula_masked_matches_the_restatement(ctx, tag):
    q = gc.problem("myula_masked", tag)
    _assert_last_sample(f"myula_masked {tag}", _myula_masked(ctx, q, q["noise"]), gc.reference("myula_masked", tag)["x"])


# ---- 2. a batch of two against the two single calls: bit for bit --------------------------------------------------------
def _same(a, b, keys, what):
    for k in keys:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=f"{k} {what}")


def _second_image(y):
    return np.ascontiguousarray(y[::-1, ::-1]) * 0.9 + 5.0


@pytest.mark.parametrize("tag", BATCH_TAGS["skrock"])
def test_skrock_batch_of_two_is_the_two_single_calls(ctx, tag):
    """Own theta, sigma2 and stream; at seam and oddM the trace ring is skrock.hip's part + slot*batch*ntv."""
    q = gc.problem("skrock", tag)
    y2 = np.stack([q["y"], _second_image(q["y"])])
    th, s2 = np.array([0.02, 0.03]), q["sigma2"] * np.array([1.0, 1.3])
    nz = np.random.default_rng(3).standard_normal((gc.STEPS, 2) + q["y"].shape)
    post = dict(first=2)
    for noise in (None, nz):
        both = _skrock(ctx, q, noise, y=y2, theta_op=th, sigma2=s2, seed=5, chain_offset=2, posterior=post)
        assert both["x"].shape == y2.shape and both["gx"].shape == (2, gc.STEPS + 1)
        for b in range(2):
            alone = _skrock(ctx, q, None if noise is None else noise[:, b], y=y2[b], theta_op=th[b], sigma2=s2[b], seed=5,
                            chain_offset=2 + b, posterior=post)
            for k in ("x", "gx", "logpi", "mean", "var"):
                np.testing.assert_array_equal(np.asarray(both[k])[b], np.asarray(alone[k]), err_msg=f"{k} chain {b}")
            assert both["count"][b] == alone["count"] == gc.STEPS
        assert both["gx"][0, 1] != both["gx"][1, 1] and np.all(np.isfinite(both["logpi"]))


def _sapg_batch(ctx, run, driver, tag, masks):
    q = gc.problem(driver, tag)
    y = q["setup"]["y"]
    y2 = np.stack([y, _second_image(y)])
    x2 = np.stack([y, 0.5 * y[::-1] + 20.0])
    nz = np.random.default_rng(3).standard_normal((q["noise"].shape[0], 2) + y.shape)
    post = dict(first=2)
    keys = SAPG_ARRAYS + tuple(n + "s" for n in NAMES_OF[q["kind"]]) + tuple("grad_" + n for n in NAMES_OF[q["kind"]]) + (
        "posteriormean", "posteriorvar")
    for noise in (None, nz):
        mk = lambda b: {} if masks is None else dict(mask=masks[b] if b is not None else masks)
        both = run(ctx, q, noise, x0=x2, y=y2, seed=5, chain_offset=2, posterior=post, **mk(None))[-1]
        assert len(both) == 2
        for b in range(2):
            alone = run(ctx, q, None if noise is None else noise[:, b], x0=x2[b], y=y2[b], seed=5, chain_offset=2 + b,
                        posterior=post, **mk(b))[-1]
            _same(both[b], alone, keys, f"chain {b}")
            for k in ("theta_EB", "sigma_EB", "posterior_count"):
                assert both[b][k] == alone[k], k
        assert both[0]["thetas"][1] != both[1]["thetas"][1] and np.all(np.isfinite(both[1]["logPiTraceX"]))


@pytest.mark.parametrize("tag", BATCH_TAGS["SAPG_skrock"])
def test_sapg_skrock_batch_of_two_is_the_two_single_calls(ctx, tag):
    """Own image, start and stream; at seam and oddM u.tvp is re-pointed every iteration at [batch][ntv] partials."""
    _sapg_batch(ctx, _sapg_skrock, "SAPG_skrock", tag, None)


@pytest.mark.parametrize("tag", BATCH_TAGS["SAPG_masked"])
def test_sapg_masked_batch_of_two_is_the_two_single_calls(ctx, tag):
    q = gc.problem("SAPG_masked", tag)
    _sapg_batch(ctx, _sapg_masked, "SAPG_masked", tag, np.stack([q["mask"], gc.OTHER_MASK[tag](q["mask"].shape)]))


@pytest.mark.parametrize("tag", BATCH_TAGS["myula_masked"])
def test_myula_masked_batch_of_two_is_the_two_single_calls(ctx, tag):
    q = gc.problem("myula_masked", tag)
    y2 = np.stack([q["y"], _second_image(q["y"])])
    m2 = np.stack([q["mask"], gc.OTHER_MASK[tag](q["mask"].shape)])
    th, s2 = q["theta"] * np.array([1.0, 1.5]), q["s2"] * np.array([1.0, 1.3])
    nz = np.random.default_rng(3).standard_normal((gc.MYULA_SAMPLES - 2, 2) + q["y"].shape)
    post = dict(first=1)
    for noise in (None, nz):
        both = _myula_masked(ctx, q, noise, y=y2, mask=m2, theta_op=th, sigma2=s2, seed=7, chain_offset=1, posterior=post)
        for b in range(2):
            alone = _myula_masked(ctx, q, None if noise is None else noise[:, b], y=y2[b], mask=m2[b], theta_op=th[b],
                                  sigma2=s2[b], seed=7, chain_offset=1 + b, posterior=post)
            for k in ("x", "mean", "var"):
                np.testing.assert_array_equal(np.asarray(both[k])[b], np.asarray(alone[k]), err_msg=f"{k} chain {b}")
            assert both["count"][b] == alone["count"] == 2
        assert np.all(np.isfinite(both["x"]))


# ---- 3. the generator at the seam ---------------------------------------------------------------------------------------
def test_philox_at_the_seam_pair_262144_draws_its_own_counter(ctx):
    """noise = NULL at 1090 x 481: the one pair of the second grid-stride trip draws (262 144, step, chain), not pair 0's
    counter: the chain is the restatement fed with the restated normals, at the standing bars."""
    q = gc.problem("skrock", "seam")
    M, N = q["y"].shape
    seed, off, pair = 11, 2, gc.EW_MAX_BLOCKS * gc.EW_LANES
    dev = phr.chain_normals(M * N, gc.STEPS, 1, seed, off)[:, 0]         # (steps, P) in device order
    assert M * N // 2 == pair + 1
    for s in range(gc.STEPS):
        assert dev[s, 2 * pair] != dev[s, 0] and dev[s, 2 * pair + 1] != dev[s, 1]
        assert abs(dev[s, 2 * pair] - dev[s, 0]) > 1e-3
    nz = phr.as_arrays(dev, M)
    a = _skrock(ctx, q, seed=seed, chain_offset=off)
    _assert_skrock("skrock seam, Philox", a, gc.chain("skrock", "seam", noise=nz))
    # and the last pair of the state is felt: with pair 0's normals there the restatement is another chain at that pixel
    wrong = dev.copy()
    wrong[:, 2 * pair:] = dev[:, :2]
    r = gc.chain("skrock", "seam", noise=phr.as_arrays(wrong, M))
    d = np.abs(phr.device_order(r["samples"][-1])[2 * pair:] - phr.device_order(np.asarray(a["x"]))[2 * pair:])
    print(f"with pair 0's normals at pair {pair} the last pair of the sample would move by {d.max():.2e}")
    assert d.max() > 1e-3


def test_philox_chains_at_the_wave_plan_match_the_restated_normals(ctx):
    """1024 x 1024: every lane draws a second pair; sbtv_SAPG_skrock counts its steps through the warm-up."""
    q = gc.problem("SAPG_skrock", "wave")
    M, N = q["setup"]["y"].shape
    nz = phr.as_arrays(phr.chain_normals(M * N, q["noise"].shape[0], 1, 11, 2), M)[:, 0]
    out = _sapg_skrock(ctx, q, seed=11, chain_offset=2)
    _assert_sapg("SAPG_skrock wave, Philox", "SAPG_skrock", out, q["kind"], gc.chain("SAPG_skrock", "wave", noise=nz))


# ---- 4. moments on the second trip --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["wave", "seam"])
def test_skrock_moments_on_the_second_trip(ctx, tag):
    q, ref = gc.problem("skrock", tag), gc.reference("skrock", tag)
    got = _skrock(ctx, q, q["noise"], posterior=dict(first=2))
    assert got["count"] == _assert_moments(f"skrock {tag}", got["mean"], got["var"], ref["samples"][1:])
    plain = _skrock(ctx, q, q["noise"])
    _same(got, plain, ("x", "gx", "logpi"), "with and without moments")


@pytest.mark.parametrize("driver,tag", [("SAPG_skrock", "seam"), ("SAPG_masked", "wave-holes"), ("SAPG_masked", "seam-valid")])
def test_sapg_moments_on_the_second_trip(ctx, driver, tag):
    q, ref = gc.problem(driver, tag), gc.reference(driver, tag)
    run = _sapg_skrock if driver == "SAPG_skrock" else _sapg_masked
    got = run(ctx, q, q["noise"], posterior=dict(first=2))[-1]
    n = _assert_moments(f"{driver} {tag}", got["posteriormean"], got["posteriorvar"], ref["samples"][1:])
    assert got["posterior_count"] == n == 2


@pytest.mark.parametrize("tag", ["wave-holes", "seam-valid"])
def test_myula_masked_moments_on_the_second_trip(ctx, tag):
    """first = 1: the chain has two states, X(1) = y and one move; first = 2 would leave one sample and no Welford update."""
    q, ref = gc.problem("myula_masked", tag), gc.reference("myula_masked", tag)
    got = _myula_masked(ctx, q, q["noise"], posterior=dict(first=1))
    assert got["count"] == _assert_moments(f"myula_masked {tag}", got["mean"], got["var"], ref["samples"]) == 2


# ---- 5. the trace ring of sbtv_skrock -----------------------------------------------------------------------------------
RING, RING_SAMPLES, RING_FIRST = 1024, 1030, 1022


def test_skrock_trace_ring_flush_and_restart(ctx):
    """16 x 16, s = 2, 1030 samples: the ring of 1024 slots is flushed at sample 1024 and restarts at slot 0 with
    ii0 = ii - filled + 1.  One call against 1022 samples and a continuation from its x with the remaining noise: the
    arithmetic is the same (skrock_perturb_nocontract is the one expression for both ways of forming P), only the slot
    bookkeeping differs, so gx, logpi and the last sample are the same bits.  The continuation's sample 1 is sample 1022
    again."""
    assert RING_FIRST < RING < RING_SAMPLES
    M, N, stages, _, seed, cit = gc.SKROCK["p16"]
    q = skc.build(M, N, stages, RING_SAMPLES - 1, seed, cit)
    nz = q["noise"]
    one = _skrock(ctx, q, nz, samples=RING_SAMPLES)
    a = _skrock(ctx, q, nz[:RING_FIRST - 1], samples=RING_FIRST)
    b = _skrock(ctx, q, nz[RING_FIRST - 1:], x0=np.asarray(a["x"]), samples=RING_SAMPLES - RING_FIRST + 1)
    assert np.all(np.isfinite(one["logpi"])) and np.all(one["gx"] > 0)
    for k in ("gx", "logpi"):
        assert b[k][0] == a[k][-1], k                                    # sample 1022, traced by both calls
        two = np.concatenate([a[k], b[k][1:]])
        assert two.shape == one[k].shape == (RING_SAMPLES,)
        for ii in (1023, 1024, 1025, 1026):                              # around the flush, by name
            assert one[k][ii - 1] == b[k][ii - RING_FIRST], (k, ii, one[k][ii - 3:ii + 2], b[k][:6])
        np.testing.assert_array_equal(one[k], two, err_msg=k)
        assert len(set(one[k][1020:].tolist())) == RING_SAMPLES - 1020  # all different: a shifted entry cannot match
    np.testing.assert_array_equal(np.asarray(one["x"]), np.asarray(b["x"]))
    # the first samples are the restatement's
    ref = skc.chain_of(dict(q, op=dict(q["op"], samples=4)))
    for k in ("gx", "logpi"):
        print(f"ring {k}[:4]: worst rel {_rel(one[k][:4], ref[k]):.1e}")
        np.testing.assert_allclose(one[k][:4], ref[k], rtol=1e-9, atol=0, err_msg=k)
    four = _skrock(ctx, q, nz, samples=4)
    _assert_last_sample("skrock ring, sample 4", four["x"], ref["samples"][-1])
    np.testing.assert_array_equal(four["gx"], one["gx"][:4])


# ---- 6. the synchronisation stride of the SAPG drivers ------------------------------------------------------------------
SYNC = dict(samples=1030, warmup=2, burnIn=2)             # 1030 steps: one synchronisation inside the loop (every 1024)


@pytest.mark.parametrize("driver", ["SAPG_skrock", "SAPG_masked"])
def test_sapg_chain_across_the_synchronisation_stride(ctx, driver):
    """16 x 16 with warmup + samples > 1024 (SAPG_SK_SYNC / SAPG_MK_SYNC): twice the same bits, finite to the end, and the
    first 8 iterations are the restatement's (delta(ii) and the updates do not depend on the length of the run)."""
    case = gc.TABLES[driver]["p16"]
    mod, run = (ssc, _sapg_skrock) if driver == "SAPG_skrock" else (msc, _sapg_masked)
    q = mod.build(gc._key(case), **SYNC)
    assert q["noise"].shape[0] == SYNC["warmup"] - 1 + SYNC["samples"] - 1 > 1024
    r1, r2 = run(ctx, q, q["noise"]), run(ctx, q, q["noise"])
    keys = SAPG_ARRAYS + tuple(n + "s" for n in NAMES_OF[q["kind"]]) + tuple("grad_" + n for n in NAMES_OF[q["kind"]])
    _same(r1[-1], r2[-1], keys, "run twice")
    assert r1[:-1] == r2[:-1]
    for k in keys:
        assert np.all(np.isfinite(np.asarray(r1[-1][k]))), k
    assert len(set(r1[-1]["logPiTraceX"][1000:].tolist())) == 30        # the chain is alive beyond the synchronisation
    n = 8
    ref = mod.chain_of(q, noise=q["noise"][:SYNC["warmup"] - 1 + n - 1], samples=n)
    _assert_sapg_traces(f"{driver} p16 x {SYNC['samples']}, first {n}", driver, r1[-1], None, q["kind"], ref, n)


# ---- 7. the figures -----------------------------------------------------------------------------------------------------
def test_report_the_worst_figures():
    """Prints what the tests above measured (run the whole file with -s); the module docstring quotes a run on an MI355X."""
    assert WORST
    for k in sorted(WORST):
        print(f"worst {k}: {WORST[k]:.1e}")
