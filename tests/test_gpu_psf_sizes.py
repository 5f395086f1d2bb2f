"""GPU: the SAPG parameter step and the device PSF taps at mask sizes other than 7 x 7 and with a rotated Gaussian, on the
cases of tests/psf_size_cases.py (tests/test_psf_sizes_cpu.py shows that they are good cases: parameters that move at every
iteration and never touch a bound, traces that do not amplify a last-bit perturbation to 1 / 100 of any bar used here).

  T1 .. T9  sbtv.SAPG_algorithm_* with injected noise against sbtv_oracle at the bars of
            tests/test_gpu_sapg_fista.py::test_sapg_matches_oracle_with_injected_noise: sapg_update_kernel's wave branch at 9, 25
            and 64 lanes and on its second trip over the spectrum sets, its block branch at 81, 121, 144 and 225 lanes,
            psf_taps_point with phi != 0 on the device, psf_spectrum_sets with three sets at other sizes than 7 (T9: the
            chirp-z twin), the Laplace alias D2s = D1s.
  W1 .. W3  sbtv.SAPG_wavelet_semiblind against tests/wavelet_sb_restatement.literal at the bars of
            tests/test_gpu_wavelet_sb.py: wav_sb_update_kernel at 81, 225 and 9 lanes, two sets of taps, g0_scale.
  The taps the update kernels left in "sapg.par" / "wsb.par" against sbtv_oracle.PSF_TAPS at the DEVICE's last parameters
  (no trajectory error enters): taps to rtol 1e-13, derivative taps to 1e-13 (|e| a + f |a'|) / a^2
  (psf_size_cases.taps_and_bars).

Measured on an MI355X (worst error as a fraction of its bar, over the chains of a case):

  case  worst trace against the oracle     taps in the workspace   device loop / host loop
        (fraction of its bar)            (sets, fraction)        (fraction of 1e-9)
  T1    gXTrace 3.8e-06                  1 set(s), 0.0022        -
  T2    gXTrace 3.0e-06                  1 set(s), 0.0022        2e-06
  T3    gXTrace 3.6e-06                  1 set(s), 0.012         1.5e-06
  T4    sigmas 1.0e-03                   1 set(s), 0.02          2.1e-05
  T5    gXTrace 2.3e-06                  1 set(s), 0.0075        2.2e-07
  T6    sigmas 1.2e-04                   -                       -
  T6 on one stream: the same traces (1.2e-04); 2 set(s), 0.0069
  T7    ps 5.6e-06                       6 set(s), 0.0024        2e-06
  T8    gXTrace 3.5e-06                  -                       -
  T9    gXTrace 4.1e-06                  1 set(s), 0.006         -
  grad_theta: at most 4.6e-04 of its bar (T4).
  W1 .. W3: every trace within 3.4e-13 relative of the restatement (bar 1e-9); taps 0.01 / 0.0091 / 0.0019 of the bar.
"""
import numpy as np
import pytest

import psf_size_cases as pc
from test_gpu_sapg_fista import _op_struct
from test_gpu_wavelet_sb import _check as _wav_check, _run as _wav_run

pytestmark = pytest.mark.gpu

TV_NAMES = sorted(pc.TV_CASES)
LANES_OFF = {"T7"}                     # six chains on ONE stream: the default policy would deal them to two lanes, 3 + 3
# (case, lanes off).  T6 twice: the default policy deals its two chains 1 + 1 to two lanes, so each update kernel sees
# nspec = 1; on one stream it is the wave branch with two spectrum sets and H, D1, D2 of their own
TV_RUNS = [(n, n in LANES_OFF) for n in TV_NAMES] + [("T6", True)]
_run_id = lambda r: r[0] + ("-one-stream" if r[1] and r[0] not in LANES_OFF else "")
_TAP_RUNS = [r for r in TV_RUNS if r[0] != "T8" and r != ("T6", False)]


@pytest.fixture()
def ctx1():
    """A context of its own with the lanes switched off (one stream), closed after the test."""
    import sbtv
    c = sbtv.Context(0)
    c.set_lanes(1)
    yield c
    c.close()


def _context(request, off):
    return request.getfixturevalue("ctx1" if off else "ctx")


def _fn(kind):
    import sbtv
    return {"gaussian": sbtv.SAPG_algorithm_Guassian, "moffat": sbtv.SAPG_algorithm_moffat,
            "laplace": sbtv.SAPG_algorithm_laplace}[kind]


def _tv_op(p):
    """The op and c structs of a case: tests/test_gpu_sapg_fista._op_struct with the case's size, rotation, start values,
    every PSF parameter free and the scaled step constants."""
    kind = p["kind"]
    op, c, names = _op_struct(kind, p["sts"][0], pc.SAMPLES, pc.WARMUP, pc.BURNIN, pc.CHAMBOLLEIT)
    op["psf_size"], op["phi"] = p["size"], p["phi"]
    for q, nm in enumerate(names):
        op[nm + "_init"] = pc.P_INIT[kind][q]
        op["fix_" + nm] = 0
        c[nm] = p["c"]["p"][q]
    if p["shared"]:
        op["chains"] = p["chains"]
    return op, c, names


def _tv_y(p):
    return p["sts"][0]["y"] if (p["shared"] or p["chains"] == 1) else np.stack([st["y"] for st in p["sts"]])


def _tv_call(cx, p, **kw):
    """One call on problem p: the list of per-chain results."""
    op, c, names = _tv_op(p)
    op.update(kw.pop("op", {}))
    res = _fn(p["kind"])(_tv_y(p), op, c, share_gradients=p["shared"], ctx=cx, **kw)[-1]
    return res if isinstance(res, list) else [res]


def _par(cx, name, t, nsets):
    """[taps | d0 | d1] of a "sapg.par" / "wsb.par" workspace as (3, nsets, t, t) arrays in the oracle's orientation (the
    workspace holds column-major masks)."""
    flat = np.asarray(cx.workspace(name, 3 * t * t * nsets, 1)).reshape(-1)
    return flat.reshape(3, nsets, t, t).transpose(0, 1, 3, 2)


_TV_RUNS = {}


def _tv_gpu(name, cx, off):
    """The injected-noise device-loop run of a case and the taps it left behind: (results per chain, par or None).  Run once per
    session on the session's context; a lanes-off run happens on the context of the test that asks."""
    if not off and name in _TV_RUNS:
        return _TV_RUNS[name]
    p = pc.tv_problem(name)
    nz = p["noise"] if p["chains"] > 1 else p["noise"][:, 0]
    res = _tv_call(cx, p, noise=nz)
    lanes = p["chains"] > 1 and not p["shared"] and not off                    # the chains ran in the lanes' own contexts
    par = None if lanes else _par(cx, "sapg.par", p["size"], 1 if p["shared"] else p["chains"])
    if not off:
        _TV_RUNS[name] = (res, par)
    return res, par


def _oracle_keys(r, names):
    """A chain's results under the keys of psf_size_cases.TV_BARS."""
    return dict(r, ps=np.stack([r[nm + "s"] for nm in names]), grads_p=np.stack([r["grad_" + nm] for nm in names]))


@pytest.mark.parametrize("name,off", TV_RUNS, ids=[_run_id(r) for r in TV_RUNS])
def test_injected_noise_parity_with_the_oracle(request, name, off):
    """(a) every assertion of test_sapg_matches_oracle_with_injected_noise; the chains of T6 / T7 against their own
    single-chain oracle runs, T8 against SAPG_algorithm_shared (with the grad_theta of
    test_sapg_shared_gradient_chains_match_oracle, here for every case)."""
    cx = _context(request, off)
    p, ref = pc.tv_problem(name), pc.tv_reference(name)
    names = pc.NAMES[p["kind"]]
    res, _ = _tv_gpu(name, cx, off)
    assert len(res) == p["chains"]
    burnIn, samples = pc.BURNIN, pc.SAMPLES
    total = {}
    for b, (r, rr) in enumerate(zip(res, ref)):
        worst = pc.tv_compare(_oracle_keys(r, names), rr, label=f"{name} chain {b}", shared=p["shared"])
        for k, (e, f) in worst.items():
            total[k] = max(total.get(k, 0.0), f)
        for q, nm in enumerate(names):
            assert r[nm + "_EB"] == pytest.approx(rr["p_EB"][q], rel=1e-8)
            assert len(set(np.asarray(r[nm + "s"]).tolist())) == samples                 # the parameter moved at every iteration
        # derived logs: mean_thetas(ii-burnIn) = mean(thetas(burnIn:ii)), tol_thetas(ii), written out as in the 7 x 7 test
        th = rr["thetas"]
        want_mean = [np.mean(th[burnIn - 1:i + 1]) for i in range(burnIn, samples)]
        np.testing.assert_allclose(r["mean_thetas"], want_mean, rtol=1e-9)
        i = samples - 1
        want_tol = abs(np.mean(th[burnIn - 1:i + 1]) - np.mean(th[burnIn - 1:i])) / np.mean(th[burnIn - 1:i])
        assert r["tol_thetas"][i] == pytest.approx(want_tol, rel=1e-6)
        assert np.isnan(r["tol_thetas"][burnIn - 1]) and r["tol_thetas"][0] == 0.0
        if p["kind"] == "moffat":
            assert r["err_psf"][0] == 0.0 and r["err_psf"][1] > 0.0
    print(f"{_run_id((name, off))}: worst fraction of its bar: " + ", ".join(f"{k} {f:.1e}" for k, f in total.items()))
    if p["shared"]:
        for r in res[1:]:
            for nm in names:
                np.testing.assert_array_equal(r[nm + "s"], res[0][nm + "s"])
        assert np.max(np.abs(res[0]["Xlast_sample"] - res[1]["Xlast_sample"])) > 1e-3


def _check_taps(label, kind, t, phi, par, params):
    """par (3, nsets, t, t) against the oracle's taps of params[set]; returns the worst error as a fraction of its bar."""
    npar = len(pc.P_INIT[kind])
    worst = 0.0
    for s, pv in enumerate(params):
        taps, dtaps, bar, dbars = pc.taps_and_bars(kind, t, pv, phi)
        for what, got, ref, b in [("taps", par[0, s], taps, bar)] + [(f"d{q}", par[1 + q, s], dtaps[q], dbars[q])
                                                                    for q in range(npar)]:
            err = np.abs(got - ref)
            frac = float(np.max(err / b))
            worst = max(worst, frac)
            assert np.all(err <= b), f"{label} set {s} {what}: {frac:.3g} of the bar at tap {np.unravel_index(np.argmax(err / b), b.shape)}"
        assert abs(float(np.sum(par[0, s])) - 1.0) <= 1e-13
        if npar == 1:
            assert np.all(par[2, s] == 0.0)                   # no second parameter: the kernel writes zeros
    return worst


@pytest.mark.parametrize("name,off", _TAP_RUNS, ids=[_run_id(r) for r in _TAP_RUNS])
def test_taps_the_update_kernel_left_behind(request, name, off):
    """(b) "sapg.par" after the device loop holds the taps and derivative taps of p(samples), per spectrum set (T6 on one
    stream: two sets; in two lanes its taps are in the lanes' own contexts)."""
    cx = _context(request, off)
    p = pc.tv_problem(name)
    names = pc.NAMES[p["kind"]]
    res, par = _tv_gpu(name, cx, off)
    params = [tuple(float(r[nm + "s"][-1]) for nm in names) for r in res]
    assert len(set(params)) == len(params)                    # T7: six chains, six pairwise different parameters
    worst = _check_taps(name, p["kind"], p["size"], p["phi"], par, params)
    print(f"{_run_id((name, off))}: taps / derivative taps of {len(params)} set(s): worst {worst:.2g} of the bar")


@pytest.mark.parametrize("name", ["T2", "T3", "T4", "T5", "T7"])
def test_device_resident_loop_matches_host_side_loop(request, name):
    """(c) Philox noise, the key list and bars of
    tests/test_gpu_sapg_fista.py::test_sapg_device_resident_loop_matches_host_side_loop."""
    cx = _context(request, name in LANES_OFF)
    p = pc.tv_problem(name)
    names = pc.NAMES[p["kind"]]
    dev = _tv_call(cx, p, op=dict(seed=5))
    host = _tv_call(cx, p, op=dict(seed=5), host_loop=True)
    keys = ["thetas", "sigmas", "logPiTraceX", "logPiTrace_WU", "gXTrace", "grad_theta", "grad_sigma", "theta_EB",
            "sigma_EB", "Xlast_sample"] + [nm + "s" for nm in names] + [nm + "_EB" for nm in names]
    worst = 0.0
    for b in range(p["chains"]):
        for key in keys:
            a, c = np.asarray(dev[b][key]), np.asarray(host[b][key])
            worst = max(worst, float(np.max(np.abs(a - c) / (1e-9 + 1e-9 * np.abs(c)))))
            np.testing.assert_allclose(a, c, rtol=1e-9, atol=1e-9, err_msg=f"{name} chain {b} {key}")
        assert any(len(set(np.asarray(dev[b][nm + "s"]).tolist())) > 1 for nm in names)     # a parameter did move
    print(f"{name}: device loop against host loop, worst {worst:.2g} of the bar")


@pytest.mark.parametrize("name", sorted(pc.WAV_CASES))
def test_wavelet_semiblind_matches_the_literal_restatement(ctx, name):
    """(d) the assertions of tests/test_gpu_wavelet_sb.py on W1 .. W3, then (b) on "wsb.par".  Its derivative taps are the
    reference's (utils/diff_moffat_alpha.m as it stands); g0_scale enters the gradient, not the taps."""
    p, ref = pc.wav_problem(name), pc.wav_reference(name)
    got = _wav_run(ctx, p, pc.wav_noise(name))
    par = _par(ctx, "wsb.par", p["psf_size"], p["batch"])
    _wav_check(got, ref, p, name)
    npar = len(p["ops"][0]["p_min"])
    params = [tuple(float(v) for v in r["ps"][:npar, -1]) for _, r in got]
    assert len(set(params)) == len(params)
    worst = _check_taps(name, p["kind"], p["psf_size"], p["phi"], par, params)
    print(f"{name}: taps / derivative taps of {len(params)} set(s): worst {worst:.2g} of the bar")


@pytest.fixture()
def fresh():
    """A context that has run nothing yet (default lane policy), closed after the test."""
    import sbtv
    c = sbtv.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("kind", ["gaussian", "moffat", "laplace"])
def test_refusals(fresh, kind):
    """(e) psf_size 0, 16, negative, larger than M, larger than N: SBTV_ERR_PSF from the entry's own guard (its message; the
    wrapper's err_psf trace would refuse 0 and 16 too, but only after the loop had run) and before any launch: the loop
    reserves its workspaces before its first launch, and on this context, which has run nothing, none exists afterwards.
    Then the context runs a valid call."""
    import sbtv
    name = {"gaussian": "T1", "moffat": "T6", "laplace": "T7"}[kind]
    p = pc.tv_problem(name)
    op, c, names = _tv_op(p)
    y = p["sts"][0]["y"]                                       # 48 x 32
    for arr, size in ((y, 0), (y, 16), (y, -3), (y[:12, :], 13), (y[:, :12], 13), (y[:14, :14], 15)):
        with pytest.raises(sbtv.SbtvError) as e:
            _fn(kind)(np.ascontiguousarray(arr), dict(op, psf_size=size), c, ctx=fresh)
        assert e.value.code == -10, (arr.shape, size, e.value.code)          # SBTV_ERR_PSF
        assert "Mask does not fit inside array" in e.value.msg, (arr.shape, size, e.value.msg)
    for ws in ("sapg.par", "sapg.X", "sapg.H"):
        with pytest.raises(sbtv.SbtvError) as e:
            fresh.workspace(ws, 1, 1)
        assert e.value.code == -1 and "no workspace named" in e.value.msg, (ws, e.value.msg)
    nz = p["noise"][:, 0]
    r = _fn(kind)(y, op, c, noise=nz, ctx=fresh)[-1]
    np.testing.assert_allclose(r["thetas"], pc.tv_reference(name)[0]["thetas"], rtol=1e-9)
    assert fresh.workspace("sapg.par", 3 * p["size"] ** 2, 1).shape == (3 * p["size"] ** 2, 1)     # now it exists
