"""GPU: semi-blind empirical Bayes for the wavelet-l1 prior (sbtv_SAPG_wavelet_semiblind, csrc/wavelet_sapg_sb.hip) against
the literal NumPy restatement (tests/wavelet_sb_restatement.py) on the cases of tests/wavelet_sb_cases.py.

Parity with injected noise: every trace, the EB estimates and max|X_last - ref| / max|X_last| to rtol 1e-9, the project's
figure for these traces (tests/test_gpu_wavelet_sapg.py); the tol_* entries, differences of two nearly equal means, absolutely
to 1e-12 where they are below 1e-9; a p entry that sits on a clamp in the reference is compared exactly.
tests/test_wavelet_sb_cpu.py shows that no case amplifies a 1e-12 perturbation beyond 1e-10 over its length, so the bound is
about arithmetic.  With every parameter fixed the chain is compared with sbtv.SAPG_wavelet; Philox chains are reproducible,
follow chain_offset and agree statistically with restatement chains (|difference of the means| <= 3 pooled standard errors,
the criterion of tests/test_gpu_sapg_long.py)."""
import functools

import numpy as np
import pytest

import wavelet_sb_cases as wbc
import wavelet_sb_restatement as wsb

pytestmark = pytest.mark.gpu

TRACES = ("thetas", "ps", "sigmas", "grads", "gXTrace", "logPiTraceX", "logPiTrace_WU", "mean_thetas", "tol_thetas",
          "mean_ps", "tol_ps")
BITS = tuple(k for k in TRACES if k != "logPiTrace_WU")


def _op(p, **opkw):
    """The op of a call on problem p: chain 0's, with one p_init row per chain."""
    op = dict(p["ops"][0], **opkw)
    if "p_init" not in opkw and p["batch"] > 1:
        op["p_init"] = np.array([o["p_init"] for o in p["ops"]])
    return op


def _run(ctx, p, nz=None, y=None, **opkw):
    """sbtv.SAPG_wavelet_semiblind on problem p (all its images in one call) as a list of (eb, results) per chain."""
    import sbtv
    op = _op(p, **opkw)
    y = p["y"] if y is None else y
    if y.shape[0] == 1:
        if np.ndim(op["p_init"]) == 2:
            op["p_init"] = op["p_init"][0]
        eb, res = sbtv.SAPG_wavelet_semiblind(y[0], p["kind"], p["h"], p["levels"], op, noise=None if nz is None else nz[:, 0],
                                              ctx=ctx)
        return [(eb, res)]
    eb, res = sbtv.SAPG_wavelet_semiblind(y, p["kind"], p["h"], p["levels"], op, noise=nz, ctx=ctx)
    return [(dict(theta=eb["theta"][b], p=eb["p"][b], sigma2=eb["sigma2"][b]), res[b]) for b in range(len(res))]


def _check(got, ref, p, label, rtol=1e-9):
    op = p["ops"][0]
    for b, ((eb, r), (eb_ref, rr)) in enumerate(zip(got, ref)):
        xs = float(np.max(np.abs(rr["Xlast_sample"])))
        ex = float(np.max(np.abs(np.asarray(r["Xlast_sample"]) - rr["Xlast_sample"])))
        print(f"{label} chain {b}: theta_EB {eb['theta']:.12g} / {eb_ref['theta']:.12g}, p_EB {eb['p']} / {eb_ref['p']}, "
              f"sigma2_EB {eb['sigma2']:.12g} / {eb_ref['sigma2']:.12g}, max|X - ref| / max|X| = {ex / xs:.1e}")
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
            if k.startswith("tol_"):
                small = fin & (np.abs(c) < 1e-9)
                assert np.all(np.abs(a[small] - c[small]) <= 1e-12), k
                fin = fin & ~small
            if k == "ps":                                     # an entry on a clamp is that bound, exactly
                for q in range(len(op["p_min"])):
                    on = (c[q] == op["p_min"][q]) | (c[q] == op["p_max"][q])
                    np.testing.assert_array_equal(a[q][on], c[q][on], err_msg="ps on a clamp")
            if k == "sigmas":
                on = (c == op["sigma2_min"]) | (c == op["sigma2_max"])
                np.testing.assert_array_equal(a[on], c[on], err_msg="sigma2 on a clamp")
            np.testing.assert_allclose(a[fin], c[fin], rtol=rtol, atol=0, err_msg=k)
        assert abs(eb["theta"] - eb_ref["theta"]) <= rtol * eb_ref["theta"]
        assert abs(eb["sigma2"] - eb_ref["sigma2"]) <= rtol * eb_ref["sigma2"]
        np.testing.assert_allclose(eb["p"], eb_ref["p"], rtol=rtol, atol=0)
        assert r["mean_theta"] == eb["theta"] and r["sigma2_EB"] == eb["sigma2"] and np.all(r["p_EB"] == eb["p"])
        assert r["last_theta"] == r["thetas"][-1] and r["last_samp"] == len(r["thetas"])
        assert ex <= rtol * xs


@pytest.mark.parametrize("name", sorted(wbc.CASES))
def test_traces_match_the_literal_restatement(ctx, name):
    """(A) 64 x 64 Haar, Laplace: b runs onto its lower bound and leaves it; (B) 100 x 90 D4, Gaussian: the chirp-z FFT path,
    the D2 spectrum, two chains with their own start values, noise and taps; (C) sigma2 free: onto sigma2_max and off it; (D)
    34 x 30 Moffat, beta fixed, a part-full last workgroup; (E) 1024 x 1024: the pipelined row kernel, OP_GRAD without store
    followed by OP_GRADF from the same spectrum."""
    p, ref = wbc.problem(name), wbc.reference(name)
    got = _run(ctx, p, wbc.noise(name))
    _check(got, ref, p, name)
    op = p["ops"][0]
    if name == "A":
        b = got[0][1]["ps"][0]
        at = np.flatnonzero(b == op["p_min"][0])
        assert at.size and np.any(b[at[-1] + 1:] > op["p_min"][0])
    if name == "C":
        s = got[0][1]["sigmas"]
        assert np.any(s == op["sigma2_max"]) and s[-1] < op["sigma2_max"]


@pytest.mark.parametrize("name", ["A", "B"])
def test_every_parameter_fixed_is_the_theta_only_entry(ctx, name):
    """Every parameter fixed at p_init = p_true against sbtv.SAPG_wavelet with the sbtv.psf_family taps of the same
    parameters: the same spectra, the same step function, sums of the same row blocks (DESIGN.md section 3.11 records whether
    the bits agree)."""
    import sbtv
    p, nz = wbc.problem(name), wbc.noise(name)
    op0 = p["ops"][0]
    npar = wsb.NPAR[p["kind"]]
    got = _run(ctx, p, nz, fix_p=(True,) * npar, p_init=op0["p_true"], fix_sigma=True)
    A = sbtv.BlurOperator(sbtv.psf_family(p["kind"], 7, op0["p_true"])[0])
    if p["batch"] == 1:
        ref = [sbtv.SAPG_wavelet(p["y"][0], A, p["h"], p["levels"], op0, noise=nz[:, 0], ctx=ctx)]
    else:
        ref = list(zip(*sbtv.SAPG_wavelet(p["y"], A, p["h"], p["levels"], op0, noise=nz, ctx=ctx)))
    for b, ((eb, r), (eb0, r0)) in enumerate(zip(got, ref)):
        bits = True
        for k in ("thetas", "gXTrace", "logPiTraceX", "tol_thetas", "mean_thetas"):
            a, c = np.asarray(r[k]), np.asarray(r0[k])
            bits = bits and np.array_equal(a, c, equal_nan=True)
            np.testing.assert_allclose(a, c, rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
        xa, xc = np.asarray(r["Xlast_sample"]), np.asarray(r0["Xlast_sample"])
        bits = bits and np.array_equal(xa, xc) and eb["theta"] == eb0
        print(f"case {name} chain {b}: bit-equal to sbtv.SAPG_wavelet: {bits}")
        assert abs(eb["theta"] - eb0) <= 1e-12 * eb0
        assert np.max(np.abs(xa - xc)) <= 1e-12 * np.max(np.abs(xc))
        assert np.all(r["ps"][:npar] == np.array(op0["p_true"])[:, None]) and np.all(r["sigmas"] == op0["sigma2"])


def test_philox_chains_are_reproducible_and_streams_follow_chain_offset(ctx):
    p = wbc.problem("B")
    one, two = _run(ctx, p, seed=5), _run(ctx, p, seed=5)
    for (eb1, r1), (eb2, r2) in zip(one, two):
        assert eb1["theta"] == eb2["theta"] and np.all(eb1["p"] == eb2["p"])
        for k in BITS:
            np.testing.assert_array_equal(r1[k], r2[k], err_msg=k)
        np.testing.assert_array_equal(np.asarray(r1["Xlast_sample"]), np.asarray(r2["Xlast_sample"]))
    assert one[0][1]["gXTrace"][0] != one[1][1]["gXTrace"][0]                      # two streams
    assert len(set(one[1][1]["ps"][0].tolist())) > 10                              # the parameters are free and move
    # chain 1 of the batch at chain_offset 0 = a call of its own at chain_offset 1, bit for bit
    (eb_a, r_a), = _run(ctx, p, y=p["y"][1:], seed=5, chain_offset=1, p_init=p["ops"][1]["p_init"])
    for k in BITS:
        np.testing.assert_array_equal(r_a[k], one[1][1][k], err_msg=k)
    np.testing.assert_array_equal(np.asarray(r_a["Xlast_sample"]), np.asarray(one[1][1]["Xlast_sample"]))
    assert eb_a["theta"] == one[1][0]["theta"] and np.all(eb_a["p"] == one[1][0]["p"])
    other = _run(ctx, p, seed=6)
    assert other[0][1]["gXTrace"][0] != one[0][1]["gXTrace"][0]


STAT_CHAINS, STAT_SAMPLES = 8, 300


@functools.lru_cache(maxsize=None)
def _stat_reference():
    """(theta_EB, b_EB) of 8 chains of the literal restatement on case A's problem, 300 samples, NumPy normals (once)."""
    p = wbc.problem("A")
    op = dict(p["ops"][0], samples=STAT_SAMPLES)
    steps = max(op["warmup"] - 1, 0) + STAT_SAMPLES - 1
    shape = (steps, p["y"].shape[1], wbc.wsc.bands(p["levels"]) * p["y"].shape[2])
    out = []
    for c in range(STAT_CHAINS):
        eb, _ = wsb.literal(p["y"][0], p["model"], p["h"], p["levels"], op, np.random.default_rng(100 + c).standard_normal(shape))
        out.append((eb["theta"], eb["p"][0]))
    return np.array(out)


def test_eb_estimates_of_philox_chains_within_the_restatement_chains_spread(ctx):
    p = wbc.problem("A")
    y8 = np.repeat(p["y"], STAT_CHAINS, axis=0)
    got = _run(ctx, p, y=y8, samples=STAT_SAMPLES, seed=7)
    gpu = np.array([(eb["theta"], eb["p"][0]) for eb, _ in got])
    ref = _stat_reference()
    n = STAT_CHAINS
    for q, what in enumerate(("theta_EB", "b_EB")):
        assert len(set(gpu[:, q].tolist())) == n                                    # all different streams
        se = np.sqrt(gpu[:, q].var(ddof=1) / n + ref[:, q].var(ddof=1) / n)
        diff = abs(gpu[:, q].mean() - ref[:, q].mean())
        print(f"{what}: device {gpu[:, q].mean():.6g} (sd {gpu[:, q].std(ddof=1):.2e}), restatement {ref[:, q].mean():.6g} "
              f"(sd {ref[:, q].std(ddof=1):.2e}), |d| = {diff:.3g} = {diff / se:.2f} SE")
        assert diff <= 3.0 * se, what


def test_device_tensors_give_the_same_bits(ctx):
    import sbtv
    p, nz = wbc.problem("B"), wbc.noise("B")
    host = _run(ctx, p, nz)
    nzd = sbtv.to_device(nz.reshape((-1,) + nz.shape[2:]))         # step-major, column-major coefficient arrays
    eb, res = sbtv.SAPG_wavelet_semiblind(sbtv.to_device(p["y"]), p["kind"], p["h"], p["levels"], _op(p), noise=nzd, ctx=ctx)
    for b in range(2):
        assert eb["theta"][b] == host[b][0]["theta"] and np.all(eb["p"][b] == host[b][0]["p"])
        for k in BITS:
            np.testing.assert_array_equal(res[b][k], host[b][1][k], err_msg=k)
        np.testing.assert_array_equal(sbtv.to_host(res[b]["Xlast_sample"]), np.asarray(host[b][1]["Xlast_sample"]))
    with pytest.raises(ValueError, match="noise"):                # the device-noise validation of SAPG_wavelet
        sbtv.SAPG_wavelet_semiblind(sbtv.to_device(p["y"]), p["kind"], p["h"], p["levels"], _op(p), noise=nzd.reshape(-1)[:-2],
                                    ctx=ctx)


def test_refusals(ctx):
    """Each is refused with its code before any GPU work, and a valid call succeeds afterwards."""
    import sbtv
    p = wbc.problem("D")
    y, h, op = p["y"][0], p["h"], p["ops"][0]
    call = lambda kind=p["kind"], arr=y, hh=h, levels=p["levels"], **kw: sbtv.SAPG_wavelet_semiblind(
        arr, kind, hh, levels, dict(op, **kw), ctx=ctx)
    inf, nan = float("inf"), float("nan")
    bad = [dict(samples=1), dict(burnIn=0), dict(burnIn=4), dict(warmup=-1), dict(sigma2=0.0), dict(gamma=0.0),
           dict(th_init=2.0), dict(th_init=1e-4), dict(min_th=0.0), dict(chain_offset=-1), {"lambda": -1.0},
           # a free parameter outside its bounds, or with a non-positive lower bound
           dict(p_init=(2.0, 3.5)), dict(p_init=(1e-3, 3.5)), dict(p_min=(0.0, 0.1)), dict(p_min=(-1.0, 0.1)),
           dict(c_p=(-1.0, 1.0)), dict(c_p=(inf, 1.0)), dict(c_p=(1.0, nan)), dict(c_sigma=-1.0), dict(c_sigma=inf),
           # a free sigma2 outside its bounds, or with a non-positive lower bound
           dict(fix_sigma=False, sigma2=op["sigma2_max"] * 2), dict(fix_sigma=False, sigma2=op["sigma2_min"] / 2),
           dict(fix_sigma=False, sigma2_min=0.0), dict(fix_sigma=False, sigma2_min=op["sigma2_max"] * 2)]
    for kw in bad:
        with pytest.raises(sbtv.SbtvError) as e:
            call(**kw)
        assert e.value.code == -1, (kw, e.value.code)
    for kw in (dict(kind=3), dict(kind=-1), dict(psf_size=0), dict(psf_size=17), dict(psf_size=31)):   # SBTV_ERR_PSF
        with pytest.raises(sbtv.SbtvError) as e:
            call(**kw)
        assert e.value.code == -10, (kw, e.value.code)                                # SBTV_ERR_PSF
    d4 = sbtv.daubcqf(4)
    for hh, levels, arr, code in ((np.array([1.0, 0.25]), 3, y, -1),                # not orthonormal
                                  (np.ones(3), 3, y, -1), (h, 1, y, -1),
                                  (d4, 4, np.ones((12, 12)), -2),                   # too small for the depth
                                  (h, 3, np.ones((33, 35)), -2)):                   # an odd pixel count
        with pytest.raises(sbtv.SbtvError) as e:
            call(arr=arr, hh=hh, levels=levels)
        assert e.value.code == code, (hh.size, levels, arr.shape, e.value.code)
    # what is only checked for a FREE parameter is accepted for a fixed one
    call(fix_p=(True, True), p_init=op["p_true"], p_min=(0.0, 0.0), p_max=(20.0, 20.0))
    eb, res = call()
    assert op["min_th"] <= eb["theta"] <= op["max_th"] and res["last_samp"] == op["samples"]
    assert op["p_min"][0] <= eb["p"][0] <= op["p_max"][0] and res["ps"][1, 1] == op["p_true"][1]

