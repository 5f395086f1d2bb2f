"""GPU: long SAPG chains (round-3 review item 1).

(a) device-resident loop against the host-side loop over 2 100 samples after 1 100 warm-up steps (both cross the
    `(ii & 1023) == 0` synchronisation of `device_loop` in csrc/sapg.hip twice, warm-up once), eager and under graph replay;
(b) oracle parity with injected noise over 320 samples at 64^2 for the three PSF families with the REFERENCE'S OWN
    step scales, so that the projections of SAPG_algorithm_Guassian.m:166-194 engage and release: whole traces, the EB
    estimates and the running-mean / tolerance logs (:217-284) against the committed oracle fixture with sigma^2 fixed;
    with sigma^2 estimated the reference's iteration is chaotic (the oracle on y (1 + 1e-12) leaves its own trajectory
    after 31-134 samples): per-step parity up to that horizon, and the whole chain in re-anchored 8-sample segments;
(c) statistical parity of the EB estimates: 16 device Philox chains against 16 oracle chains with
    NumPy noise (fixture), |difference of the means| <= 3 standard errors for theta, every PSF parameter and sigma^2.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import sapg_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def op_struct(kind, st, samples, warmup, burnIn, free=True):
    """The demo's `op` / `c` structs (run_*_demo.m) with the reference's step scales; free = every PSF parameter is
    estimated (the Gaussian demo's fix flags lifted, init 0.5 / 0.3, run_Gaussian_demo.m:68-69)."""
    import sbtv_oracle as o
    d = o.DEMO[kind]
    names = sc.NAMES[kind]
    fr = sc.FREE[kind] if free else dict(fix=None, p_init=None)
    init = d["init"] if fr["p_init"] is None else fr["p_init"]
    fix = d["fix"] if fr["fix"] is None else fr["fix"]
    op = dict(samples=samples, warmup=warmup, burnIn=burnIn, chambolleit=25, psf_size=7, phi=0.0,
              gamma=st["gamma"], th_init=st["th_init"], min_th=1e-3, max_th=1.0,
              sigma=st["sigma"], sigma_init=st["sigma_init"], sigma_min=st["sigma_min"], sigma_max=st["sigma_max"],
              d_scale=0.01 / st["th_init"], d_exp=0.8, fix_sigma=0)
    op["lambda"] = st["lam"]
    for q, nm in enumerate(names):
        op[nm] = st["p_true"][q]
        op[nm + "_init"] = init[q]
        op["min_" + nm] = d["pmin"][q]
        op["max_" + nm] = d["pmax"][q]
        op["fix_" + nm] = int(fix[q])
    c = dict(theta=d["c_theta"], sigma=d["c_sigma"], lam=1.0, gam=1.0)
    for q, nm in enumerate(names):
        c[nm] = d["c_p"][q]
    return op, c, names


def sapg_fn(kind):
    import sbtv
    return {"gaussian": sbtv.SAPG_algorithm_Guassian, "moffat": sbtv.SAPG_algorithm_moffat,
            "laplace": sbtv.SAPG_algorithm_laplace}[kind]


@pytest.fixture(scope="module")
def fx():
    with np.load(sc.FIXTURE) as f:
        return {k: f[k] for k in f.files}


# ---------------------------------------------------------------------------------------------------------------
# (b) per-step parity over 320 samples, reference step scales, projections active
# ---------------------------------------------------------------------------------------------------------------
def _bounds(st, d, names):
    lo, hi = min(st["sigma_min"], st["sigma_max"]), max(st["sigma_min"], st["sigma_max"])
    return lo, hi, [(d["pmin"][q], d["pmax"][q]) for q in range(len(names))]


def _check_traces(res, out, fx, t, names, n, rtol, whole):
    """Traces of the first n samples against the fixture entry t; whole = also the end-of-chain quantities."""
    s = slice(0, n)
    np.testing.assert_allclose(res["thetas"][s], fx[f"{t}.thetas"][s], rtol=rtol)
    np.testing.assert_allclose(res["sigmas"][s], fx[f"{t}.sigmas"][s], rtol=rtol)
    for q, nm in enumerate(names):
        np.testing.assert_allclose(res[nm + "s"][s], fx[f"{t}.ps"][q][s], rtol=10 * rtol)
        g_ref = fx[f"{t}.grads"][1 + q][s]
        np.testing.assert_allclose(res["grad_" + nm][1:n], g_ref[1:], rtol=1e-6, atol=1e-6 * np.max(np.abs(g_ref)))
    g_ref = fx[f"{t}.grads"][0][s]
    np.testing.assert_allclose(res["grad_theta"][1:n], g_ref[1:], rtol=10 * rtol, atol=rtol * np.max(np.abs(g_ref)))
    g_ref = fx[f"{t}.grads"][len(names) + 1][s]
    np.testing.assert_allclose(res["grad_sigma"][1:n], g_ref[1:], rtol=100 * rtol, atol=10 * rtol * np.max(np.abs(g_ref)))
    np.testing.assert_allclose(res["logPiTraceX"][s], fx[f"{t}.logPi"][s], rtol=rtol)
    np.testing.assert_allclose(res["logPiTrace_WU"][1:], fx[f"{t}.logPi_WU"][1:], rtol=1e-9)
    np.testing.assert_allclose(res["gXTrace"][:n - 1], fx[f"{t}.gX"][:n - 1], rtol=rtol)
    np.testing.assert_allclose(res["err_psf"][s], fx[f"{t}.err_psf"][s], rtol=1e-6, atol=1e-18)
    if not whole:
        return
    np.testing.assert_allclose(res["Xlast_sample"], fx[f"{t}.X"], rtol=10 * rtol, atol=10 * rtol)
    # EB estimates (:258-284) and the logs the reference keeps while iterating (:217-244)
    eb = fx[f"{t}.eb"]
    assert out[0] == pytest.approx(eb[0], rel=rtol)
    for q, nm in enumerate(names):
        assert res[nm + "_EB"] == pytest.approx(eb[1 + q], rel=10 * rtol)
    assert out[-2] == pytest.approx(eb[-1], rel=rtol)
    np.testing.assert_allclose(res["mean_thetas"], fx[f"{t}.mean_thetas"], rtol=rtol)
    np.testing.assert_allclose(res["mean_sigmas"], fx[f"{t}.mean_sigmas"], rtol=rtol)
    b = sc.TRACE["burnIn"]
    for got, want in ((res["tol_thetas"], fx[f"{t}.tol_thetas"]), (res["tol_sigma"], fx[f"{t}.tol_sigma"])):
        assert got[0] == 0.0 and np.all(np.isnan(got[1:b])) and np.all(np.isnan(want[1:b]))
        np.testing.assert_allclose(got[b:], want[b:], rtol=1e-5, atol=1e-13)


@pytest.mark.parametrize("host_loop", [False, True], ids=["device_loop", "host_loop"])
@pytest.mark.parametrize("kind", sc.KINDS)
def test_sapg_320_samples_fixed_sigma_reference_step_scales_whole_traces(ctx, fx, kind, host_loop):
    """op.fix_sigma = 1, everything else free, the reference's step scales: the PSF projections bounce between their
    bounds on every sample (Laplace), engage and release (Moffat) or both (Gaussian); the chain is stable, so ALL 320
    samples, the EB estimates and the mean_* / tol_* logs are compared.  Tolerance: 1e-9, or 30 x what a 1e-12 relative
    change of y does to the oracle itself (`sens` of the fixture) where that is larger (Moffat: 3.7e-9)."""
    import sbtv_oracle as o
    st = sc.setup(kind)
    T = sc.TRACE
    op, c, names = op_struct(kind, st, T["samples"], T["warmup"], T["burnIn"])
    op["fix_sigma"] = 1
    op["sigma_init"] = st["sigma"] ** 2          # sigma_init = op.sigma^2 when fixed (SAPG_algorithm_Guassian.m:49-53)
    out = sapg_fn(kind)(st["y"], op, c, noise=sc.trace_noise(kind), host_loop=host_loop)
    res = out[-1]
    t = f"trace_fs.{kind}"
    d = o.DEMO[kind]
    _, _, pb = _bounds(st, d, names)
    on = [(fx[f"{t}.ps"][q] == pb[q][0]) | (fx[f"{t}.ps"][q] == pb[q][1]) for q in range(len(names))]
    # engaged and released again - or (Laplace) thrown from one bound to the other on every sample
    assert all(m.sum() >= 6 for m in on)
    assert all(np.any(np.diff(m.astype(int)) == -1) or
               (np.any(fx[f"{t}.ps"][q] == pb[q][0]) and np.any(fx[f"{t}.ps"][q] == pb[q][1])) for q, m in enumerate(on))
    for q, nm in enumerate(names):
        gp = np.asarray(res[nm + "s"])
        np.testing.assert_array_equal((gp == pb[q][0]) | (gp == pb[q][1]), on[q])        # the same samples, exactly
    rtol = max(1e-9, 30 * float(fx[f"{t}.sens"].max()))
    assert rtol < 1e-8
    assert np.all(np.asarray(res["sigmas"]) == st["sigma"] ** 2)
    _check_traces(res, out, fx, t, names, T["samples"], rtol, whole=True)


@pytest.mark.parametrize("host_loop", [False, True], ids=["device_loop", "host_loop"])
@pytest.mark.parametrize("kind", sc.KINDS)
def test_sapg_all_free_reference_step_scales_up_to_the_sensitivity_horizon(ctx, fx, kind, host_loop):
    """Everything estimated, sigma^2 included, the reference's step scales.  The sigma^2 recursion then overshoots and
    jumps between its bounds and amplifies rounding differences ~2x per sample: the ORACLE run on y (1 + 1e-12) differs
    from itself by > 1e-10 from sample `horizon` on (31 / 114 / 134) and by O(1) after ~200 (fixture `sens`).  Per-step
    parity at 1e-9 is asserted up to the horizon - inside it the PSF parameters and sigma^2 all hit their bounds (the
    Gaussian widths leave theirs only around sample 130) - and the rest of the chain is covered by the re-anchored
    segments of the next test."""
    import sbtv_oracle as o
    st = sc.setup(kind)
    T = sc.TRACE
    op, c, names = op_struct(kind, st, T["samples"], T["warmup"], T["burnIn"])
    out = sapg_fn(kind)(st["y"], op, c, noise=sc.trace_noise(kind), host_loop=host_loop)
    res = out[-1]
    t = f"trace.{kind}"
    d = o.DEMO[kind]
    h = int(fx[f"{t}.horizon"])
    assert 30 <= h < T["samples"] and fx[f"{t}.sens"][-40:].max() > 1e-3          # the chain IS chaotic later on
    lo, hi, pb = _bounds(st, d, names)
    on_s = ((fx[f"{t}.sigmas"] == lo) | (fx[f"{t}.sigmas"] == hi))[:h]
    on_p = [((fx[f"{t}.ps"][q] == pb[q][0]) | (fx[f"{t}.ps"][q] == pb[q][1]))[:h] for q in range(len(names))]
    released = lambda m: bool(np.any(np.diff(m.astype(int)) == -1))
    assert on_s.any() and all(m.any() for m in on_p)                   # sigma^2 and every PSF parameter hit a bound ...
    assert released(on_s) or any(released(m) for m in on_p)            # ... and something left it again inside the horizon
    gs = np.asarray(res["sigmas"])[:h]
    np.testing.assert_array_equal((gs == lo) | (gs == hi), on_s)
    for q, nm in enumerate(names):
        gp = np.asarray(res[nm + "s"])[:h]
        np.testing.assert_array_equal((gp == pb[q][0]) | (gp == pb[q][1]), on_p[q])
    _check_traces(res, out, fx, t, names, h, 1e-9, whole=False)


SEG = 8          # samples between two re-anchorings


@pytest.mark.parametrize("kind", sc.KINDS)
def test_sapg_all_free_chain_in_re_anchored_segments_matches_oracle(ctx, kind):
    """The whole 320-sample all-free chain of the previous test, beyond its sensitivity horizon: every SEG samples the
    device chain is re-started from the ORACLE's state (X, theta, p, sigma^2 of the long oracle chain; `op.X0`,
    `iter_offset` so that delta(i) continues) and both run the next SEG updates on the same injected noise - 40 short
    chains that tile the long one, each within 1e-9 / 1e-8 of the oracle, whatever the chaos does over 320 samples."""
    import sbtv_oracle as o
    st = sc.setup(kind)
    T = sc.TRACE
    S, W = T["samples"], T["warmup"]
    nz = sc.trace_noise(kind)
    fr = sc.FREE[kind]
    starts = list(range(1, S, SEG))                               # 1-based iteration number a segment starts FROM
    it = iter(nz)
    long = o.SAPG_algorithm(st, samples=S, warmup=W, burnIn=T["burnIn"], randn=lambda s: next(it), fix=fr["fix"],
                            p_init=fr["p_init"], keep_X=set(starts))
    d = o.DEMO[kind]
    names = sc.NAMES[kind]
    worst = 0.0
    hit = 0
    for s in starts:
        L = min(SEG, S - s)
        seg_nz = nz[W - 1 + (s - 1): W - 1 + (s - 1) + L]
        th, ps, sg = long["thetas"][s - 1], long["ps"][:, s - 1], long["sigmas"][s - 1]
        sts = dict(st, th_init=th)
        it2 = iter(seg_nz)
        ref = o.SAPG_algorithm(sts, samples=L + 1, warmup=0, burnIn=1, randn=lambda z: next(it2), fix=fr["fix"],
                               p_init=tuple(ps), sigma_init=sg, X0=long["X_at"][s], iter_offset=s - 1)
        # the segment is the long chain's continuation but for the theta of its first prox (theta(s) instead of theta(s-1))
        assert ref["thetas"][1] == pytest.approx(long["thetas"][s], rel=0.2)
        op, c, _ = op_struct(kind, sts, L + 1, 0, 1)
        op["d_scale"], op["iter_offset"], op["sigma_init"], op["X0"] = st["d_scale"], s - 1, sg, long["X_at"][s]
        for q, nm in enumerate(names):
            op[nm + "_init"] = ps[q]
        res = sapg_fn(kind)(st["y"], op, c, noise=seg_nz)[-1]
        np.testing.assert_allclose(res["thetas"], ref["thetas"], rtol=1e-9, err_msg=f"segment from {s}")
        np.testing.assert_allclose(res["sigmas"], ref["sigmas"], rtol=1e-8, err_msg=f"segment from {s}")
        for q, nm in enumerate(names):
            np.testing.assert_allclose(res[nm + "s"], ref["ps"][q], rtol=1e-8, err_msg=f"segment from {s}")
            hit += int(np.sum((ref["ps"][q][1:] == d["pmin"][q]) | (ref["ps"][q][1:] == d["pmax"][q])))
        np.testing.assert_allclose(res["logPiTraceX"], ref["logPiTraceX"], rtol=1e-9, err_msg=f"segment from {s}")
        np.testing.assert_allclose(res["Xlast_sample"], ref["Xlast_sample"], rtol=1e-8, atol=1e-8)
        worst = max(worst, float(np.max(np.abs(res["sigmas"] - ref["sigmas"]) / ref["sigmas"])))
    print(kind, len(starts), "segments, worst relative sigma^2 difference", worst, "| PSF samples on a bound:", hit)
    assert hit > 0


# ---------------------------------------------------------------------------------------------------------------
# (a) 1 100 warm-up + 2 100 samples: device-resident loop == host-side loop
# ---------------------------------------------------------------------------------------------------------------
LONG = dict(samples=2100, warmup=1100, burnIn=1680)
_TRACES = ("thetas", "sigmas", "logPiTraceX", "gXTrace", "grad_theta", "grad_sigma")


def _long_run(kind, free, host_loop, seed=5, fix_sigma=False):
    st = sc.setup(kind)
    op, c, names = op_struct(kind, st, LONG["samples"], LONG["warmup"], LONG["burnIn"], free=free)
    op["seed"] = seed
    if fix_sigma:
        op["fix_sigma"], op["sigma_init"] = 1, st["sigma"] ** 2
    out = sapg_fn(kind)(st["y"], op, c, host_loop=host_loop)            # device Philox noise in both loops
    return out, names


def test_long_chain_fixed_psf_device_loop_is_bit_equal_to_host_loop(ctx):
    """The Gaussian demo as shipped (fix_w1 = fix_w2 = 1): nothing but theta and sigma^2 moves, and the device loop
    performs the host loop's operations one for one -> every trace bit for bit after 3 198 MYULA steps."""
    (dev, names), (host, _) = _long_run("gaussian", False, False), _long_run("gaussian", False, True)
    rd, rh = dev[-1], host[-1]
    assert len(rd["thetas"]) == LONG["samples"] > 2 * 1024 and LONG["warmup"] > 1024
    for k in _TRACES + ("logPiTrace_WU", "w1s", "w2s", "Xlast_sample"):
        np.testing.assert_array_equal(rd[k], rh[k], err_msg=k)
    assert dev[0] == host[0] and dev[-2] == host[-2]                 # theta_EB, sigma_EB: means over 1680..2100
    assert np.all(np.diff(rd["thetas"][-400:]) != 0.0)               # the chain was still moving at the end


@pytest.mark.parametrize("kind", ["moffat", "laplace"])
def test_long_chain_moving_psf_device_loop_matches_host_loop(ctx, kind):
    """Estimated PSF parameters: the device loop rebuilds the taps with the device's exp / pow, the host loop with the
    host's -> equal to rounding, and the coupling of the two chains (same Philox normals) must not drift apart.
    sigma^2 is held fixed (op.fix_sigma): with the reference's c.sigma its recursion is chaotic for the first few
    hundred samples (previous tests) and two loops that differ in the last bit of a tap end up on different chains."""
    (dev, names), (host, _) = _long_run(kind, True, False, fix_sigma=True), _long_run(kind, True, True, fix_sigma=True)
    rd, rh = dev[-1], host[-1]
    for k in ("thetas", "sigmas", "logPiTraceX"):
        np.testing.assert_allclose(rd[k], rh[k], rtol=1e-9, err_msg=k)
    for nm in names:
        np.testing.assert_allclose(rd[nm + "s"], rh[nm + "s"], rtol=1e-9, err_msg=nm)
        assert rd[nm + "_EB"] == pytest.approx(rh[nm + "_EB"], rel=1e-9)
    np.testing.assert_allclose(rd["Xlast_sample"], rh["Xlast_sample"], rtol=1e-8, atol=1e-8)
    assert dev[0] == pytest.approx(host[0], rel=1e-10) and dev[-2] == pytest.approx(host[-2], rel=1e-10)


GRAPH_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(%(root)r, "semi-blind-image-deblurring-problems-with-tv_amd"))
sys.path.insert(0, os.path.join(%(root)r, "oracle"))
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import test_gpu_sapg_long as t
out = {}
for kind, free in (("gaussian", False), ("laplace", True)):
    res, names = t._long_run(kind, free, False)
    r = res[-1]
    for k in ("thetas", "sigmas", "logPiTraceX", "logPiTrace_WU", "Xlast_sample") + tuple(n + "s" for n in names):
        out[kind + "." + k] = np.asarray(r[k])
    out[kind + ".eb"] = np.array([res[0], res[-2]])
import sbtv
out["switches"] = np.array(sbtv.switches())
np.savez(sys.argv[1], **out)
"""


def test_long_chain_under_graph_replay_equals_eager_launches(tmp_path):
    """SBTV_GRAPH=1 (read once per process -> child processes): the iteration body captured once and replayed 1 097 +
    2 098 times, across both synchronisation points, gives the eager loop's traces bit for bit."""
    got = {}
    for name, env in (("eager", {}), ("graph", {"SBTV_GRAPH": "1"})):
        path = str(tmp_path / (name + ".npz"))
        e = dict(os.environ)
        e.update(env)
        subprocess.run([sys.executable, "-c", GRAPH_CHILD % {"root": ROOT}, path], check=True, env=e, timeout=900)
        got[name] = np.load(path)
    assert "SBTV_GRAPH" in str(got["graph"]["switches"]) and "SBTV_GRAPH" not in str(got["eager"]["switches"])
    for k in got["eager"].files:
        if k != "switches":
            np.testing.assert_array_equal(got["graph"][k], got["eager"][k], err_msg=k)


# ---------------------------------------------------------------------------------------------------------------
# (c) statistical parity of the EB estimates
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sc.KINDS)
def test_eb_estimates_of_philox_chains_within_the_oracle_chains_spread(ctx, fx, kind):
    """16 independent device chains (ONE batched call on 16 copies of the observation, Philox streams 0..15) against the 16
    oracle chains of the fixture (NumPy normals): same observation, same step scales, different noise."""
    st = sc.setup(kind)
    S = sc.STAT
    op, c, names = op_struct(kind, st, S["samples"], S["warmup"], S["burnIn"])
    op["seed"] = 7
    y8 = np.repeat(st["y"][None], S["chains"], axis=0)
    out = sapg_fn(kind)(y8, op, c)
    res = out[-1]
    gpu = np.array([[r["theta_EB"]] + [r[nm + "_EB"] for nm in names] + [r["sigma_EB"]] for r in res])
    ref = fx[f"stat.{kind}.eb"]
    assert gpu.shape == ref.shape == (S["chains"], len(names) + 2)
    assert len({r["theta_EB"] for r in res}) == S["chains"]                 # all different streams
    n = S["chains"]
    se = np.sqrt(gpu.var(0, ddof=1) / n + ref.var(0, ddof=1) / n)
    diff = np.abs(gpu.mean(0) - ref.mean(0))
    labels = ["theta"] + list(names) + ["sigma2"]
    report = ", ".join(f"{l}: |d| {d:.3g} = {d / s:.2f} SE" for l, d, s in zip(labels, diff, se))
    print(kind, report)
    assert np.all(diff <= 3.0 * se), report
    # and the spreads themselves are of the same order (a chain that ignored its noise would pass the test above)
    ratio = gpu.std(0, ddof=1) / ref.std(0, ddof=1)
    assert np.all((ratio > 0.2) & (ratio < 5.0)), ratio
