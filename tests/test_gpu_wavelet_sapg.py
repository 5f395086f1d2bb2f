"""GPU: the empirical-Bayes estimate of theta for the wavelet-l1 prior (sbtv_SAPG_wavelet, csrc/wavelet_sapg.hip) against the
literal NumPy restatement of SALSA/SAPG_algorithm_1.m (tests/wavelet_sapg_restatement.py) on the cases of
tests/wavelet_sapg_cases.py.

Parity with injected noise: every trace and theta_EB to rtol 1e-9, the figure of the trace tests of sbtv_SAPG_algorithm
(tests/test_gpu_sapg_fista.py); tol_thetas, a difference of two nearly equal means, absolutely to 1e-12 where it is below
1e-9; the last sample to 1e-9 max|X|.  The chain is not chaotic (a 1e-12 perturbation of case a's start is 4e-12 after 300
samples on the CPU), so no sensitivity horizon is needed.  Statistics: 8 Philox chains against 8 restatement chains with NumPy
normals, |difference of the mean theta_EB| <= 3 pooled standard errors, the criterion of tests/test_gpu_sapg_long.py."""
import functools

import numpy as np
import pytest

import wavelet_sapg_cases as wsc
import wavelet_sapg_restatement as wsr

pytestmark = pytest.mark.gpu

TRACES = ("thetas", "gXTrace", "logPiTraceX", "logPiTrace_WU", "mean_thetas", "tol_thetas")


def _blur(p):
    import sbtv
    return sbtv.BlurOperator(sbtv.psf_family("gaussian", p["psf_size"], wsc.wc.PSF_PARAMS)[0])


def _run(ctx, p, nz=None, y=None, **opkw):
    """sbtv.SAPG_wavelet on problem p (all its images in one call), as a list of (theta_EB, results) per chain."""
    import sbtv
    op = dict(p["op"], **opkw)
    y = p["y"] if y is None else y
    if y.shape[0] == 1:
        eb, res = sbtv.SAPG_wavelet(y[0], _blur(p), p["h"], p["levels"], op, noise=None if nz is None else nz[:, 0], ctx=ctx)
        return [(eb, res)]
    eb, res = sbtv.SAPG_wavelet(y, _blur(p), p["h"], p["levels"], op, noise=nz, ctx=ctx)
    return list(zip(eb, res))


def _check(got, ref, label):
    for b, ((eb, r), (eb_ref, rr)) in enumerate(zip(got, ref)):
        xs = float(np.max(np.abs(rr["Xlast_sample"])))
        ex = float(np.max(np.abs(np.asarray(r["Xlast_sample"]) - rr["Xlast_sample"])))
        print(f"{label} chain {b}: theta_EB {eb:.12g} / {eb_ref:.12g} (rel {abs(eb / eb_ref - 1):.1e}), "
              f"max|X - ref| / max|X| = {ex / xs:.1e}")
        for k in TRACES:
            if k not in rr:
                assert k not in r
                continue
            a, c = np.asarray(r[k], dtype=np.float64), np.asarray(rr[k], dtype=np.float64)
            assert a.shape == c.shape, (k, a.shape, c.shape)
            fin = np.isfinite(c)
            np.testing.assert_array_equal(np.isnan(a), np.isnan(c), err_msg=k)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(c[fin] != 0, np.abs(a[fin] / c[fin] - 1), np.abs(a[fin]))
            print(f"    {k}: {a.size} entries, {np.sum(~fin)} NaN, worst rel {rel.max() if rel.size else 0:.1e}")
            if k == "tol_thetas":
                small = fin & (np.abs(c) < 1e-9)
                assert np.all(np.abs(a[small] - c[small]) <= 1e-12), k
                fin = fin & ~small
            np.testing.assert_allclose(a[fin], c[fin], rtol=1e-9, atol=0, err_msg=k)
        assert abs(eb - eb_ref) <= 1e-9 * eb_ref
        assert r["mean_theta"] == eb and r["last_theta"] == r["thetas"][-1] and r["last_samp"] == len(r["thetas"])
        assert ex <= 1e-9 * xs


@pytest.mark.parametrize("name", sorted(wsc.CASES))
def test_traces_match_the_literal_restatement(ctx, name):
    """(a) 64 x 64 Haar with a warm-up, theta visits both bounds; (b) 100 x 90 D4: the chirp-z FFT path, no warm-up, two
    chains in one call with their own noise; (c) 34 x 30, one step: the last sample is the element-wise kernel's output on
    7140 coefficients; (d) 2 x 2; (e) 1024 x 1024: the pipelined row kernel and the grid-stride loop."""
    p, ref = wsc.problem(name), wsc.reference(name)
    _check(_run(ctx, p, wsc.noise(name)), ref, name)


def test_philox_chains_are_reproducible_and_streams_follow_chain_offset(ctx):
    p = wsc.problem("b")
    one, two = _run(ctx, p, seed=5), _run(ctx, p, seed=5)
    for (eb1, r1), (eb2, r2) in zip(one, two):
        assert eb1 == eb2
        for k in TRACES[:3] + TRACES[4:]:
            np.testing.assert_array_equal(r1[k], r2[k], err_msg=k)
        np.testing.assert_array_equal(np.asarray(r1["Xlast_sample"]), np.asarray(r2["Xlast_sample"]))
    assert one[0][1]["gXTrace"][0] != one[1][1]["gXTrace"][0]                      # two streams
    # chain 1 of the batch at chain_offset 0 = a call of its own at chain_offset 1
    alone = _run(ctx, p, y=p["y"][1:], seed=5, chain_offset=1)
    _check(alone, [one[1]], "offset")
    other = _run(ctx, p, seed=6)
    assert other[0][1]["gXTrace"][0] != one[0][1]["gXTrace"][0]


STAT_CHAINS, STAT_SAMPLES = 8, 300


@functools.lru_cache(maxsize=None)
def _stat_reference():
    """theta_EB of 8 chains of the literal restatement on case a's problem, 300 samples, NumPy normals (computed once)."""
    p = wsc.problem("a")
    op = dict(p["op"], samples=STAT_SAMPLES)
    steps = max(op["warmup"] - 1, 0) + STAT_SAMPLES - 1
    shape = (steps, p["y"].shape[1], wsc.bands(p["levels"]) * p["y"].shape[2])
    return np.array([wsr.sapg_wavelet_literal(p["y"][0], p["H"], p["h"], p["levels"], op,
                                              np.random.default_rng(100 + c).standard_normal(shape))[0]
                     for c in range(STAT_CHAINS)])


def test_theta_eb_of_philox_chains_within_the_restatement_chains_spread(ctx):
    p = wsc.problem("a")
    y8 = np.repeat(p["y"], STAT_CHAINS, axis=0)
    gpu = np.array([eb for eb, _ in _run(ctx, p, y=y8, samples=STAT_SAMPLES, seed=7)])
    ref = _stat_reference()
    assert len(set(gpu.tolist())) == STAT_CHAINS                                    # all different streams
    n = STAT_CHAINS
    se = np.sqrt(gpu.var(ddof=1) / n + ref.var(ddof=1) / n)
    diff = abs(gpu.mean() - ref.mean())
    print(f"theta_EB: device {gpu.mean():.6g} (spread {gpu.std(ddof=1) / gpu.mean():.2e}), restatement {ref.mean():.6g} "
          f"(spread {ref.std(ddof=1) / ref.mean():.2e}), |d| = {diff:.3g} = {diff / se:.2f} SE")
    assert diff <= 3.0 * se


def test_refusals(ctx):
    """Each is refused with its code before any GPU work, and a valid call succeeds afterwards."""
    import sbtv
    p = wsc.problem("c")
    A, y, h = _blur(p), p["y"][0], p["h"]
    bad_op = [dict(samples=1), dict(burnIn=0), dict(burnIn=3), dict(warmup=-1), dict(sigma2=0.0, sigma=0.0),
              dict(gamma=0.0), dict(th_init=2.0), dict(th_init=1e-4), dict(min_th=0.0), dict(chain_offset=-1)]
    bad_op.append({"lambda": -1.0})
    for kw in bad_op:
        with pytest.raises(sbtv.SbtvError) as e:
            sbtv.SAPG_wavelet(y, A, h, p["levels"], dict(p["op"], **kw), ctx=ctx)
        assert e.value.code == -1, (kw, e.value.code)
    d4 = sbtv.daubcqf(4)
    for hh, levels, arr, code in ((np.array([1.0, 0.25]), 3, y, -1),                # not orthonormal
                                  (np.sqrt(2.0) * np.array([0.75, 0.25]), 3, y, -1),
                                  (np.ones(3), 3, y, -1), (h, 1, y, -1),
                                  (d4, 4, np.ones((12, 12)), -2),                   # too small for the depth
                                  (h, 3, np.ones((33, 35)), -2)):                   # an odd pixel count
        with pytest.raises(sbtv.SbtvError) as e:
            sbtv.SAPG_wavelet(arr, A, hh, levels, p["op"], ctx=ctx)
        assert e.value.code == code, (hh.size, levels, arr.shape, e.value.code)
    eb, res = sbtv.SAPG_wavelet(y, A, h, p["levels"], p["op"], ctx=ctx)
    assert p["op"]["min_th"] <= eb <= p["op"]["max_th"] and res["last_samp"] == p["op"]["samples"]


def test_device_tensors_give_the_same_bits(ctx):
    import sbtv
    p, nz = wsc.problem("b"), wsc.noise("b")
    host = _run(ctx, p, nz)
    nzd = sbtv.to_device(nz.reshape((-1,) + nz.shape[2:]))         # step-major, column-major coefficient arrays
    eb, res = sbtv.SAPG_wavelet(sbtv.to_device(p["y"]), _blur(p), p["h"], p["levels"], p["op"], noise=nzd, ctx=ctx)
    for b in range(2):
        assert eb[b] == host[b][0]
        for k in TRACES[:3] + TRACES[4:]:
            np.testing.assert_array_equal(res[b][k], host[b][1][k], err_msg=k)
        np.testing.assert_array_equal(sbtv.to_host(res[b]["Xlast_sample"]), np.asarray(host[b][1]["Xlast_sample"]))


def test_device_noise_that_is_not_the_expected_dense_float64_array_is_refused(ctx):
    """The step kernel reads steps * B * dimX doubles from a device noise pointer, so the host mirror refuses a tensor that
    is too short, too long, float32 or strided before anything is launched; the right one still runs."""
    import sbtv
    p, nz = wsc.problem("c"), wsc.noise("c")
    yd, A = sbtv.to_device(p["y"][0]), _blur(p)
    good = sbtv.to_device(nz[:, 0])
    call = lambda t: sbtv.SAPG_wavelet(yd, A, p["h"], p["levels"], p["op"], noise=t, ctx=ctx)
    flat = good.permute(0, 2, 1).contiguous().reshape(-1)
    for bad in (flat[:-2], flat.repeat(2), flat.float(), flat.repeat(2)[::2]):
        with pytest.raises(ValueError, match="noise"):
            call(bad)
    eb, res = call(good)
    eb_flat, _ = call(flat)
    assert eb == eb_flat == _run(ctx, p, nz)[0][0]
